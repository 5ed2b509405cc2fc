#!/usr/bin/env python3
"""Extract the one Poseidon hash answer the reference ships into tests/golden/poseidon_kats.json:
   primitives/src/merkle_tree/field_based_mht/mod.rs   MNT4753_PHANTOM_MERKLE_ROOT and the sentence of its test
The constant is MNT4PoseidonHash::evaluate of ONE element: the sentence, zero-padded to 96 bytes and read little-endian; its
twelve words are the Montgomery form to 2^768 (field_new! takes the in-memory form).  Data only: the sentence and the words
(hex).  Run in the authoring container; the output is committed and nothing at run time reads the reference.
Test infrastructure."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/primitives/src"


def main():
    src = open(os.path.join(REF, "merkle_tree", "field_based_mht", "mod.rs")).read()
    m = re.search(r"pub const MNT4753_PHANTOM_MERKLE_ROOT: MNT4753Fr =\s*field_new!\(MNT4753Fr, BigInteger768\(\[(.*?)\]\)\);", src, re.S)
    words = [int(t.strip(), 0) for t in re.sub(r"//[^\n]*", "", m.group(1)).split(",") if t.strip()]
    assert len(words) == 12 and all(0 <= w < 1 << 64 for w in words)
    sentences = set(re.findall(r'let magic_string = b"([^"\\]*)";', src))
    assert len(sentences) == 1
    sentence = sentences.pop()
    assert len(sentence) == 81 and sentence in src[:m.start()]            # the comment above the constant quotes it as well
    J = {"mnt4753_phantom_merkle_root": {"tag": "mnt4753", "sentence": sentence, "input_bytes": 96,
                                         "words_montgomery_2p768": [hex(w) for w in words]}}
    out = os.path.join(HERE, "poseidon_kats.json")
    json.dump(J, open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
