"""The argument checks of include/ginger_hip.h as a table: bad calls, several per entry point, chosen so that the ORDER of the
checks shows (null arguments, handle, curve, device, ...), each with the status and the gh_last_error() text it gets.

tests/golden/abi_errors.json holds two expected columns, "no_device" and "device".  Without a device an entry point still runs
every check it makes before the device is needed, which then answers GH_E_NO_DEVICE; the wire-format checks and a few curve
checks sit behind that and show their own answer only on a device.  Rows that need a resident key exist in the device column
only.  Every row is an argument error (or an early return): none launches a kernel.

The columns are recorded from a build, not written by hand:
    python tests/test_abi_errors.py --record        (fills the column of the machine it runs on, keeps the other)
A "bad handle" is a null pointer or a zeroed buffer of 512 bytes (larger than either handle struct); a freed handle or a handle
of the other kind is never passed (undefined behaviour)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_errors.json")
SENTINEL = b"window must be 0 (auto) or in [2, 24]"     # what gh_msm_set_window(1) leaves in gh_last_error()


class Ctx:
    """Buffers the rows point at.  `big` is as large as anything a row could read or write if a check let it through."""

    def __init__(self, lib, device):
        self.lib = lib
        vp = ctypes.c_void_p
        self.zeroed = ctypes.create_string_buffer(512)           # a "handle" that fails the magic check
        self.big = np.zeros((1 << 15) * 12 + 12, np.uint64)      # 2^15 field elements + 1 (the 2-adicity rows: 3 MB)
        self.big_b = np.zeros_like(self.big)
        self.big_c = np.zeros_like(self.big)
        self.big_out = np.zeros_like(self.big)
        self.small = np.zeros(1024, np.uint64)                   # a point, a scalar, a few field elements
        self.out = np.zeros(1024, np.uint64)
        self.byte = np.zeros(16, np.uint8)
        self.handle_out = vp()
        with open(os.path.join(ROOT, "tests", "golden", "constants.json")) as f:
            p4 = int(json.load(f)["fields"]["p4"]["p"], 16)
        self.wire_inf2 = np.zeros(193, np.uint8)
        self.wire_inf2[192] = 2
        self.wire_modulus = np.zeros(193, np.uint8)
        self.wire_modulus[:96] = np.frombuffer(p4.to_bytes(96, "little"), np.uint8)
        self.key0 = self.key2 = None
        if device:       # keys without bases: a live handle that no kernel was launched for
            self.key0, self.key2 = vp(), vp()
            assert lib.gh_bases_upload(0, None, None, 0, ctypes.byref(self.key0)) == 0
            assert lib.gh_bases_upload(2, None, None, 0, ctypes.byref(self.key2)) == 0
            self.pair_same = (vp * 2)(self.key0, self.key0)
            self.pair_mixed = (vp * 2)(self.key0, self.key2)
        self.pair_null = (vp * 2)(None, None)
        self.pair_zeroed = (vp * 2)(ctypes.addressof(self.zeroed), ctypes.addressof(self.zeroed))
        self.ptrs = (vp * 2)(self.small.ctypes.data, self.small.ctypes.data)
        self.sizes0 = (ctypes.c_size_t * 2)(0, 0)
        self.sizes1 = (ctypes.c_size_t * 2)(1, 1)
        self.null_ptrs = (vp * 2)(None, None)

    def close(self):
        for k in (self.key0, self.key2):
            if k is not None:
                assert self.lib.gh_bases_free(k) == 0


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def rows():
    """(name, where, call): where is "both" or "device"; call(lib, c) returns the entry point's return value."""
    Z = lambda c: ctypes.addressof(c.zeroed)
    H = lambda c: ctypes.byref(c.handle_out)
    R = []

    def add(name, call, where="both"):
        R.append((name, where, call))

    # ---- gh_init / settings
    add("init: device index 99", lambda l, c: l.gh_init((ctypes.c_int * 1)(99), 1))
    add("set_window 1", lambda l, c: l.gh_msm_set_window(1))
    add("set_window 25", lambda l, c: l.gh_msm_set_window(25))
    add("set_window -1", lambda l, c: l.gh_msm_set_window(-1))
    add("set_affine 3", lambda l, c: l.gh_msm_set_affine(3))
    add("set_affine -1", lambda l, c: l.gh_msm_set_affine(-1))
    add("key_cache_config table_after -1", lambda l, c: l.gh_key_cache_config(1 << 30, -1))
    add("key_cache_stats null", lambda l, c: l.gh_key_cache_stats(None))
    add("batch_timing index -1", lambda l, c: l.gh_msm_batch_timing(-1, None))
    add("batch_timing index 100000", lambda l, c: l.gh_msm_batch_timing(100000, None))
    add("get_window curve 9 (value)", lambda l, c: l.gh_msm_get_window(9, 1 << 20))
    # ---- gh_msm, gh_msm_cached
    for fn in ("gh_msm", "gh_msm_cached"):
        add(fn + ": null out, curve 9", lambda l, c, fn=fn: getattr(l, fn)(9, P(c.small), None, 1, P(c.small), 1, None))
        add(fn + ": null bases", lambda l, c, fn=fn: getattr(l, fn)(0, None, None, 1, P(c.small), 1, P(c.out)))
        add(fn + ": null scalars", lambda l, c, fn=fn: getattr(l, fn)(0, P(c.small), None, 1, None, 1, P(c.out)))
        add(fn + ": curve 9", lambda l, c, fn=fn: getattr(l, fn)(9, P(c.small), None, 1, P(c.small), 1, P(c.out)))
        add(fn + ": curve -1", lambda l, c, fn=fn: getattr(l, fn)(-1, P(c.small), None, 1, P(c.small), 1, P(c.out)))
    # ---- keys
    add("bases_upload: null out, curve 9", lambda l, c: l.gh_bases_upload(9, P(c.small), None, 1, None))
    add("bases_upload: null bases", lambda l, c: l.gh_bases_upload(0, None, None, 1, H(c)))
    add("bases_upload: curve 9", lambda l, c: l.gh_bases_upload(9, P(c.small), None, 1, H(c)))
    add("upload_wire: null out, curve 7", lambda l, c: l.gh_bases_upload_wire(7, P(c.wire_inf2), 1, None))
    add("upload_wire: null bytes", lambda l, c: l.gh_bases_upload_wire(0, None, 1, H(c)))
    add("upload_wire: curve 7", lambda l, c: l.gh_bases_upload_wire(7, P(c.wire_inf2), 1, H(c)))
    add("upload_wire: infinity byte 2", lambda l, c: l.gh_bases_upload_wire(0, P(c.wire_inf2), 1, H(c)))
    add("upload_wire: coordinate = modulus", lambda l, c: l.gh_bases_upload_wire(0, P(c.wire_modulus), 1, H(c)))
    add("generate_chain: null p0, curve 9", lambda l, c: l.gh_bases_generate_chain(9, None, P(c.small), 4, H(c)))
    add("generate_chain: null out", lambda l, c: l.gh_bases_generate_chain(0, P(c.small), P(c.small), 4, None))
    add("generate_chain: n = 2^40, curve 9", lambda l, c: l.gh_bases_generate_chain(9, P(c.small), P(c.small), 1 << 40, H(c)))
    add("generate_chain: curve 9", lambda l, c: l.gh_bases_generate_chain(9, P(c.small), P(c.small), 4, H(c)))
    add("key_id: null out", lambda l, c: l.gh_bases_key_id(0, P(c.small), None, 1, None))
    add("key_id: null bases", lambda l, c: l.gh_bases_key_id(0, None, None, 1, ctypes.cast(P(c.out), ctypes.POINTER(ctypes.c_uint64))))
    add("content_hash: null bases (value)", lambda l, c: l.gh_bases_content_hash(0, None, None, 1, None))
    for name, h in (("null", lambda c: None), ("zeroed", Z)):
        add("bases_free: %s handle" % name, lambda l, c, h=h: l.gh_bases_free(h(c)))
        add("bases_len: %s handle (value)" % name, lambda l, c, h=h: l.gh_bases_len(h(c)))
        add("bases_table_rows: %s handle (value)" % name, lambda l, c, h=h: l.gh_bases_table_rows(h(c)))
        add("bases_precomputed_window: %s handle (value)" % name, lambda l, c, h=h: l.gh_bases_precomputed_window(h(c)))
        add("precompute: %s handle, window 1" % name, lambda l, c, h=h: l.gh_bases_precompute(h(c), 1))
        add("precompute_rows: %s handle, window 25, max_rows -1" % name, lambda l, c, h=h: l.gh_bases_precompute_rows(h(c), 25, -1))
        add("bases_download: %s handle, null out" % name, lambda l, c, h=h: l.gh_bases_download(h(c), 0, 1, None))
        add("msm_resident: %s handle, null scalars" % name, lambda l, c, h=h: l.gh_msm_resident(h(c), None, 1, None))
        add("msm_resident_dev: %s handle, null out" % name, lambda l, c, h=h: l.gh_msm_resident_dev(h(c), None, 1, None))
        add("fixed_base_msm: %s table, null scalars" % name, lambda l, c, h=h: l.gh_fixed_base_msm(h(c), None, 1, None))
        add("fixed_base_msm_affine: %s table, null scalars" % name, lambda l, c, h=h: l.gh_fixed_base_msm_affine(h(c), None, 1, None, None, 0))
        add("fixed_base_free: %s table" % name, lambda l, c, h=h: l.gh_fixed_base_free(h(c)))
    K = lambda c: c.key0
    add("precompute_rows: key, window 1", lambda l, c: l.gh_bases_precompute_rows(K(c), 1, 0), "device")
    add("precompute_rows: key, window 25", lambda l, c: l.gh_bases_precompute_rows(K(c), 25, 0), "device")
    add("precompute_rows: key, window -1", lambda l, c: l.gh_bases_precompute_rows(K(c), -1, 0), "device")
    add("precompute_rows: key, max_rows -1", lambda l, c: l.gh_bases_precompute_rows(K(c), 0, -1), "device")
    add("precompute_rows: key, window 1 and max_rows -1", lambda l, c: l.gh_bases_precompute_rows(K(c), 1, -1), "device")
    add("bases_len: key (value)", lambda l, c: l.gh_bases_len(K(c)), "device")
    add("bases_table_rows: key (value)", lambda l, c: l.gh_bases_table_rows(K(c)), "device")
    add("bases_download: key, count 0", lambda l, c: l.gh_bases_download(K(c), 5, 0, None), "device")
    add("bases_download: key, range outside", lambda l, c: l.gh_bases_download(K(c), 1, 1, P(c.out)), "device")
    add("bases_download: key, null out", lambda l, c: l.gh_bases_download(K(c), 0, 1, None), "device")
    add("msm_resident: key, null out", lambda l, c: l.gh_msm_resident(K(c), P(c.small), 1, None), "device")
    add("msm_resident: key, null scalars", lambda l, c: l.gh_msm_resident(K(c), None, 1, P(c.out)), "device")
    add("msm_resident_dev: key, null out", lambda l, c: l.gh_msm_resident_dev(K(c), P(c.small), 1, None), "device")
    add("msm_resident_dev: key, null scalars", lambda l, c: l.gh_msm_resident_dev(K(c), None, 1, P(c.out)), "device")
    # ---- gh_msm_resident_dev_batch
    add("batch: count -1", lambda l, c: l.gh_msm_resident_dev_batch(c.pair_zeroed, c.ptrs, c.sizes0, -1, P(c.out)))
    add("batch: count 0, all null", lambda l, c: l.gh_msm_resident_dev_batch(None, None, None, 0, None))
    add("batch: count 1, null handles", lambda l, c: l.gh_msm_resident_dev_batch(None, c.ptrs, c.sizes0, 1, P(c.out)))
    add("batch: count 1, null out", lambda l, c: l.gh_msm_resident_dev_batch(c.pair_zeroed, c.ptrs, c.sizes0, 1, None))
    add("batch: count 2, null handle entries", lambda l, c: l.gh_msm_resident_dev_batch(c.pair_null, c.ptrs, c.sizes0, 2, P(c.out)))
    add("batch: count 2, zeroed handles, null scalar entries", lambda l, c: l.gh_msm_resident_dev_batch(c.pair_zeroed, c.null_ptrs, c.sizes1, 2, P(c.out)))
    add("batch: mixed curves", lambda l, c: l.gh_msm_resident_dev_batch(c.pair_mixed, c.ptrs, c.sizes0, 2, P(c.out)), "device")
    add("batch: mixed curves, null scalar entries", lambda l, c: l.gh_msm_resident_dev_batch(c.pair_mixed, c.null_ptrs, c.sizes1, 2, P(c.out)), "device")
    add("batch: one curve, null scalar entries", lambda l, c: l.gh_msm_resident_dev_batch(c.pair_same, c.null_ptrs, c.sizes1, 2, P(c.out)), "device")
    # ---- transforms
    add("fft: null out", lambda l, c: l.gh_fft(1, P(c.small), 1, None, 31, 0))
    add("fft: null in", lambda l, c: l.gh_fft(1, None, 1, P(c.big_out), 31, 0))
    add("fft: log_n 31", lambda l, c: l.gh_fft(1, P(c.small), 1, P(c.big_out), 31, 0))
    add("fft: log_n at the 2-adicity", lambda l, c: l.gh_fft(1, P(c.big), 1, P(c.big_out), 15, 0))
    add("fft: field 7", lambda l, c: l.gh_fft(7, P(c.big), 1, P(c.big_out), 4, 0))
    add("fft_dev: null data", lambda l, c: l.gh_fft_dev(1, None, 4, 0))
    wm = lambda l, c, f, a, ln, d1: l.gh_witness_map(f, a, P(c.big_b), P(c.big_c), ln, d1, P(c.small), P(c.small), P(c.big_out))
    add("witness_map: null a, log_n 31", lambda l, c: wm(l, c, 1, None, 31, P(c.small)))
    add("witness_map: null d1", lambda l, c: wm(l, c, 1, P(c.big), 4, None))
    add("witness_map: log_n 31", lambda l, c: wm(l, c, 1, P(c.big), 31, P(c.small)))
    add("witness_map: log_n at the 2-adicity", lambda l, c: wm(l, c, 1, P(c.big), 15, P(c.small)))
    add("witness_map: field 7", lambda l, c: wm(l, c, 7, P(c.big), 4, P(c.small)))
    add("witness_map_dev: null a", lambda l, c: l.gh_witness_map_dev(1, None, None, None, 4, P(c.small), P(c.small), P(c.small), None))
    sw = lambda l, c, f, a, ln, d1: l.gh_sap_witness_map(f, a, P(c.big_c), ln, d1, P(c.small), P(c.big_out))
    add("sap_witness_map: null a, log_n 31", lambda l, c: sw(l, c, 1, None, 31, P(c.small)))
    add("sap_witness_map: null d1", lambda l, c: sw(l, c, 1, P(c.big), 4, None))
    add("sap_witness_map: log_n 31", lambda l, c: sw(l, c, 1, P(c.big), 31, P(c.small)))
    add("sap_witness_map: log_n at the 2-adicity", lambda l, c: sw(l, c, 1, P(c.big), 15, P(c.small)))
    add("sap_witness_map: field 7", lambda l, c: sw(l, c, 7, P(c.big), 4, P(c.small)))
    add("sap_witness_map_dev: null a", lambda l, c: l.gh_sap_witness_map_dev(1, None, None, 4, P(c.small), P(c.small), None))
    add("lagrange: null tau, log_n 31", lambda l, c: l.gh_lagrange_coefficients(1, 31, None, P(c.big_out)))
    add("lagrange: null out", lambda l, c: l.gh_lagrange_coefficients(1, 4, P(c.small), None))
    add("lagrange: log_n 31", lambda l, c: l.gh_lagrange_coefficients(1, 31, P(c.small), P(c.big_out)))
    add("lagrange: log_n at the 2-adicity", lambda l, c: l.gh_lagrange_coefficients(1, 15, P(c.small), P(c.big_out)))
    add("lagrange: field 7", lambda l, c: l.gh_lagrange_coefficients(7, 4, P(c.small), P(c.big_out)))
    add("lagrange_dev: null out, log_n 31", lambda l, c: l.gh_lagrange_coefficients_dev(1, 31, P(c.small), None))
    add("lagrange_dev: log_n 31", lambda l, c: l.gh_lagrange_coefficients_dev(1, 31, P(c.small), P(c.small)))
    add("batch_inverse: n 0, null a", lambda l, c: l.gh_batch_inverse(1, None, 0))
    add("batch_inverse: null a", lambda l, c: l.gh_batch_inverse(1, None, 4))
    add("batch_inverse: field 7", lambda l, c: l.gh_batch_inverse(7, P(c.big), 4))
    add("batch_inverse_dev: null a", lambda l, c: l.gh_batch_inverse_dev(1, None, 4))
    add("vec_mul: n 0, null a", lambda l, c: l.gh_vec_mul(1, None, None, 0))
    add("vec_mul: null b", lambda l, c: l.gh_vec_mul(1, P(c.big), None, 4))
    add("vec_mul: field 7", lambda l, c: l.gh_vec_mul(7, P(c.big), P(c.big_b), 4))
    add("vec_scale: n 0, null a", lambda l, c: l.gh_vec_scale(1, None, None, 0))
    add("vec_scale: null scalar", lambda l, c: l.gh_vec_scale(1, P(c.big), None, 4))
    add("vec_scale: field 7", lambda l, c: l.gh_vec_scale(7, P(c.big), P(c.small), 4))
    add("vec_mul_dev: null b", lambda l, c: l.gh_vec_mul_dev(1, P(c.small), None, 4))
    add("vec_scale_dev: null scalar", lambda l, c: l.gh_vec_scale_dev(1, P(c.small), None, 4))
    # ---- device buffers
    add("dev_alloc: null", lambda l, c: l.gh_dev_alloc(None, 16))
    add("dev_free: null", lambda l, c: l.gh_dev_free(None))
    add("dev_upload: 0 bytes, null", lambda l, c: l.gh_dev_upload(None, None, 0))
    add("dev_upload: null", lambda l, c: l.gh_dev_upload(None, P(c.small), 16))
    add("dev_download: null", lambda l, c: l.gh_dev_download(P(c.out), None, 16))
    add("measure_fpmul_peak: null", lambda l, c: l.gh_measure_fpmul_peak(None))
    # ---- single points
    add("proj_add: null, curve 9", lambda l, c: l.gh_proj_add(9, None, P(c.small)))
    add("proj_add: curve 9", lambda l, c: l.gh_proj_add(9, P(c.out), P(c.small)))
    add("proj_mul: null out, curve 9", lambda l, c: l.gh_proj_mul(9, P(c.small), P(c.small), None))
    add("proj_mul: curve 9", lambda l, c: l.gh_proj_mul(9, P(c.small), P(c.small), P(c.out)))
    add("proj_neg: null, curve 9", lambda l, c: l.gh_proj_neg(9, None))
    add("proj_neg: curve 9", lambda l, c: l.gh_proj_neg(9, P(c.out)))
    add("proj_to_affine: null flag, curve 9", lambda l, c: l.gh_proj_to_affine(9, P(c.small), P(c.out), None))
    add("proj_to_affine: curve 9", lambda l, c: l.gh_proj_to_affine(9, P(c.small), P(c.out), P(c.byte)))
    # ---- fixed base
    ft = lambda l, c, curve, g, ssz, w, out: l.gh_fixed_base_table(curve, g, ssz, w, out)
    add("fixed_base_table: null g, window 0", lambda l, c: ft(l, c, 0, None, 753, 0, H(c)))
    add("fixed_base_table: null out", lambda l, c: ft(l, c, 0, P(c.small), 753, 4, None))
    add("fixed_base_table: window 0, curve 9", lambda l, c: ft(l, c, 9, P(c.small), 753, 0, H(c)))
    add("fixed_base_table: window 23", lambda l, c: ft(l, c, 0, P(c.small), 753, 23, H(c)))
    add("fixed_base_table: scalar_size 0", lambda l, c: ft(l, c, 0, P(c.small), 0, 4, H(c)))
    add("fixed_base_table: scalar_size 769", lambda l, c: ft(l, c, 0, P(c.small), 769, 4, H(c)))
    add("fixed_base_table: curve 9", lambda l, c: ft(l, c, 9, P(c.small), 753, 4, H(c)))
    return R


def run_table(lib, device):
    """name -> [return value, gh_last_error() text or None]; the text is kept for negative statuses only."""
    c = Ctx(lib, device)
    got = {}
    try:
        for name, where, call in rows():
            if where == "device" and not device:
                continue
            assert lib.gh_msm_set_window(1) == -1 and lib.gh_last_error() == SENTINEL      # a known text before every row
            rc = int(call(lib, c))
            value_row = name.endswith("(value)")
            msg = lib.gh_last_error().decode() if rc < 0 and not value_row else None
            got[name] = [rc, msg]
            assert c.handle_out.value is None, name          # no row may have produced a handle
    finally:
        c.close()
    return got


def check(lib, column, device):
    with open(GOLDEN) as f:
        want = json.load(f)[column]
    got = run_table(lib, device)
    assert sorted(got) == sorted(want)
    bad = ["%s: got %r, expected %r" % (k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not bad, "\n".join(bad)


def test_core_abi_argument_errors_without_device(gl):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the device column is checked by the gpu test")
    check(gl.load_library(), "no_device", False)


@pytest.mark.gpu
def test_core_abi_argument_errors_on_device(gpu):
    check(gpu.load_library(), "device", True)


if __name__ == "__main__":       # --record: fill this machine's column from the library of this tree
    assert sys.argv[1:] == ["--record"], __doc__
    sys.path.insert(0, ROOT)
    from __graft_entry__ import _load_pkg
    mod = _load_pkg()
    lib = mod.load_library()
    device = lib.gh_init(None, 0) == 0
    data = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            data = json.load(f)
    data["device" if device else "no_device"] = run_table(lib, device)
    with open(GOLDEN, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d rows (%s)" % (len(data["device" if device else "no_device"]), "device" if device else "no device"))
