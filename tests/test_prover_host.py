"""The Python prover layer (ginger-lib_amd/prover.py, groth16.py, gm17.py) without a GPU, against a stand-in for the binding
that the key classes receive as `gl`: device buffers are host memory with bounds, resident bases are counted, the MSM calls
record (key, number of scalars, bytes of the scalar rows) and return fixed points.  What is checked is ownership -- nothing
stays on the device after a failure, the caller's buffers are never freed -- and that the two forms of the Groth16 MSM stage
hand the same work to the device."""
import ctypes
import importlib
import struct
import types

import numpy as np
import pytest

DEG = {"mnt4753_g1": 1, "mnt4753_g2": 2, "mnt6753_g1": 1, "mnt6753_g2": 3}
PAIRINGS = ("mnt4753", "mnt6753")


class Boom(RuntimeError):
    pass


def make_gl():
    """a fresh stand-in; gl.live_buffers / gl.live_bases / gl.jobs are what the tests read, gl.fail_* what they set"""
    gl = types.SimpleNamespace(live_buffers=[], live_bases=0, uploads=0, jobs=[], fail_upload=0, fail_precompute=False, fail_msm=False,
                               FIELDS={"mnt4753_fr": 0, "mnt6753_fr": 1})

    class GingerHipError(RuntimeError):
        pass

    def span(ptr, nbytes):
        """the address of [ptr, ptr + nbytes) after checking that it lies inside one live buffer"""
        addr = ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr)
        for buf in gl.live_buffers:
            if buf.ptr.value <= addr and addr + nbytes <= buf.ptr.value + buf.nbytes:
                return addr
        raise AssertionError("access outside every live device buffer")

    class DeviceBuffer:
        def __init__(self, nbytes):
            self.nbytes = int(nbytes)
            self._mem = ctypes.create_string_buffer(max(1, self.nbytes))
            self.ptr = ctypes.c_void_p(ctypes.addressof(self._mem))
            gl.live_buffers.append(self)

        def upload(self, arr):
            arr = np.ascontiguousarray(arr)
            ctypes.memmove(span(self.ptr, arr.nbytes), arr.ctypes.data, arr.nbytes)
            return self

        def download(self, dtype=np.uint64):
            return np.frombuffer(ctypes.string_at(span(self.ptr, self.nbytes), self.nbytes), dtype=dtype).copy()

        def free(self):
            if self in gl.live_buffers:
                gl.live_buffers.remove(self)
                self.ptr = ctypes.c_void_p()

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.free()

    class ResidentBases:
        def __init__(self, curve, bases, infinity=None):
            bases = np.ascontiguousarray(bases, dtype=np.uint64)
            assert bases.size % (24 * DEG[curve]) == 0
            self._make(curve, bases.size // (24 * DEG[curve]))
            assert infinity is None or len(infinity) == self.n

        @classmethod
        def from_wire(cls, curve, data):
            rec = 192 * DEG[curve] + 1
            assert len(data) % rec == 0
            self = cls.__new__(cls)
            self._make(curve, len(data) // rec)
            return self

        def _make(self, curve, n):
            gl.uploads += 1
            if gl.uploads == gl.fail_upload:
                raise Boom("upload %d" % gl.uploads)
            self.curve, self.n, self.serial, self.live = curve, n, gl.uploads, True
            gl.live_bases += 1

        def precompute(self, window_bits=0, max_rows=0):
            if gl.fail_precompute:
                raise GingerHipError("no memory for the table")
            return 13

        def download(self, first, count):
            return np.arange(count * 24 * DEG[self.curve], dtype=np.uint64).reshape(count, -1) + 1

        def msm_dev(self, d_scalars, n_scalars):
            return msm_batch_dev([(self, d_scalars, n_scalars)])[0]

        def free(self):
            if self.live:
                self.live = False
                gl.live_bases -= 1

    def msm_batch_dev(jobs):
        if gl.fail_msm:
            raise Boom("msm")
        out = []
        for rb, buf, n in jobs:
            assert rb.live
            gl.jobs.append(((rb.curve, rb.n, rb.serial), int(n), ctypes.string_at(span(buf.ptr, int(n) * 96), int(n) * 96)))
            out.append(np.full(36 * DEG[rb.curve], rb.serial, dtype=np.uint64))
        return out

    def gh_dev_upload(dst, src, nbytes):
        ctypes.memmove(span(dst, nbytes), src, nbytes)
        return 0

    def check(rc):
        if rc:
            raise GingerHipError("status %d" % rc)
    ok = lambda *args: 0
    lib = types.SimpleNamespace(gh_dev_upload=gh_dev_upload, gh_dev_sync=ok, gh_witness_map_dev=ok, gh_sap_witness_map_dev=ok, gh_vec_scale_dev=ok)
    gl.__dict__.update(
        GingerHipError=GingerHipError, DeviceBuffer=DeviceBuffer, ResidentBases=ResidentBases, msm_batch_dev=msm_batch_dev,
        load_library=lambda: lib, _check=check, _ptr=lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None,
        proj_add=lambda curve, acc, p: np.array(acc, dtype=np.uint64), proj_mul=lambda curve, xyz, k: np.array(xyz, dtype=np.uint64),
        proj_neg=lambda curve, xyz: np.array(xyz, dtype=np.uint64), field_one=lambda curve: np.ones(12 * DEG[curve], dtype=np.uint64),
        proj_to_affine=lambda curve, xyz: (np.zeros(24 * DEG[curve], dtype=np.uint64), False))
    return gl


@pytest.fixture(scope="module")
def mods(gl):
    return importlib.import_module("ginger_lib_amd.groth16"), importlib.import_module("ginger_lib_amd.gm17")


NI, N_AUX = 3, 5                          # the `Benchmark` circuit with 5 constraints: 3 inputs, 5 aux variables, domain 8
N, N_H = NI + N_AUX, 7


def groth16_arrays(pairing):
    deg = DEG[pairing + "_g2"]
    pts = lambda n, words: np.arange(n * words, dtype=np.uint64).reshape(n, words) + 1
    return {"a_query": pts(N, 24), "b_g1_query": pts(N, 24), "b_g2_query": pts(N, 24 * deg), "h_query": pts(N_H, 24), "l_query": pts(N_AUX, 24),
            "alpha_g1": pts(1, 24)[0], "beta_g1": pts(1, 24)[0], "delta_g1": pts(1, 24)[0] + 5,
            "beta_g2": pts(1, 24 * deg)[0], "delta_g2": pts(1, 24 * deg)[0]}


def groth16_blob(pairing):
    """a Parameters::write stream of the same shape (groth16/mod.rs:188-208) with zero records"""
    deg = DEG[pairing + "_g2"]
    g1, g2 = bytes(193), bytes(192 * deg + 1)
    vec = lambda rec, n: struct.pack(">I", n) + rec * n
    return (bytes(192 * deg) + g2 + g2 + vec(g1, NI) + g1 + g1 + g2 + g1 + g2 +
            vec(g1, N) + vec(g1, N) + vec(g2, N) + vec(g1, N_H) + vec(g1, N_AUX))


def gm17_arrays(pairing):
    deg = DEG[pairing + "_g2"]
    pts = lambda n, words: np.arange(n * words, dtype=np.uint64).reshape(n, words) + 1
    return {"a_query": pts(N, 24), "b_query": pts(N, 24 * deg), "c_query_1": pts(N - NI, 24), "c_query_2": pts(N, 24), "g_gamma2_z_t": pts(N_H, 24),
            "g_gamma_z": pts(1, 24)[0], "g_ab_gamma_z": pts(1, 24)[0], "g_gamma2_z2": pts(1, 24)[0], "h_gamma_z": pts(1, 24 * deg)[0],
            "a_query_inf": np.zeros(N, dtype=np.uint8)}


def constructors(mods):
    """(name, number of uploads it makes, gl -> key) for the three ways a resident key comes to be"""
    groth16, gm17 = mods
    return [("groth16 arrays", 5, lambda gl, p: groth16.ResidentProvingKey(gl, p, groth16_arrays(p), NI)),
            ("groth16 stream", 6, lambda gl, p: groth16.ResidentProvingKey.from_parameters(gl, p, groth16_blob(p), NI)),     # + delta_g1 as one point
            ("gm17 arrays", 5, lambda gl, p: gm17.ResidentGm17Key(gl, p, gm17_arrays(p), NI))]


# ---- (a) the constructors
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_a_failed_upload_leaves_nothing_on_the_device(mods, pairing):
    for name, uploads, make in constructors(mods):
        for k in range(1, uploads + 1):
            gl = make_gl()
            gl.fail_upload = k
            with pytest.raises(Boom):
                make(gl, pairing)
            assert gl.uploads == k and gl.live_bases == 0, (name, k)
        gl = make_gl()
        key = make(gl, pairing)                                   # and without a failure: five queries, gone after free()
        assert gl.uploads == uploads and gl.live_bases == 5 and len(key.keys) == 5
        key.free()
        assert gl.live_bases == 0
        key.free()                                                # twice is harmless
        assert gl.live_bases == 0


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_a_failed_precompute_is_swallowed(mods, pairing):
    for name, _, make in constructors(mods):
        gl = make_gl()
        gl.fail_precompute = True
        with make(gl, pairing) as key:
            assert gl.live_bases == 5 and len(key.keys) == 5, name
        assert gl.live_bases == 0, name                           # __exit__ is free()
        key = make(gl, pairing)
        key.close()
        assert gl.live_bases == 0, name


def scalars(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 12), dtype=np.uint64)


# ---- (b) the MSM stage fails
@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("extra_aux", [0, 2])
def test_b_groth16_stage_failure_frees_what_the_method_allocated(mods, pairing, extra_aux):
    groth16, _ = mods
    gl = make_gl()
    key = groth16.ResidentProvingKey(gl, pairing, groth16_arrays(pairing), NI)
    inp, aux, h, rs = scalars(NI - 1, 1), scalars(N_AUX + extra_aux, 2), scalars(N_H, 3), scalars(2, 4)
    gl.fail_msm = True
    with pytest.raises(Boom):                                     # host scalars, h from the host: everything is the method's own
        key.create_proof_msms(inp, aux, h[:NI], h[NI:], rs[0], rs[1])
    assert gl.live_buffers == []
    d_h = gl.DeviceBuffer((N_H + 2) * 96).upload(h)
    with pytest.raises(Boom):                                     # host scalars, h on the device: h stays
        key.create_proof_msms(inp, aux, None, None, rs[0], rs[1], h_dev=(d_h, N_H))
    assert gl.live_buffers == [d_h]
    d_s = gl.DeviceBuffer((N - 1 + 4) * 96).upload(np.concatenate([inp, aux[:N_AUX]]))
    with pytest.raises(Boom):                                     # scalars on the device: both stay
        key.create_proof_msms(None, None, None, None, rs[0], rs[1], h_dev=(d_h, N_H), scalars_dev=(d_s, N - 1))
    assert gl.live_buffers == [d_h, d_s] and d_h.ptr and d_s.ptr
    gl.fail_msm = False
    key.create_proof_msms(None, None, None, None, rs[0], rs[1], h_dev=(d_h, N_H), scalars_dev=(d_s, N - 1))
    key.create_proof_msms(inp, aux, h[:NI], h[NI:], rs[0], rs[1])
    assert gl.live_buffers == [d_h, d_s]                          # the same on the way out of a proof that succeeds


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_b_gm17_stage_failure_frees_what_the_method_allocated(mods, pairing):
    _, gm17 = mods
    gl = make_gl()
    key = gm17.ResidentGm17Key(gl, pairing, gm17_arrays(pairing), NI)
    inp, aux, h = scalars(NI - 1, 1), scalars(N - NI, 2), scalars(N_H, 3)
    d_h = gl.DeviceBuffer((N_H + 1) * 96).upload(h)
    for fail in (True, False):
        gl.fail_msm = fail
        for kw in ({}, {"h_dev": (d_h, N_H)}):
            if fail:
                with pytest.raises(Boom):
                    key.create_proof_msms(inp, aux, h, 11, 12, 13, **kw)
            else:
                key.create_proof_msms(inp, aux, h, 11, 12, 13, **kw)
            assert gl.live_buffers == [d_h] and d_h.ptr, (fail, kw)
    assert len(gl.jobs) == 10                                     # two proofs of five MSMs went through


# ---- (c) one stage behind both forms
@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("extra_aux", [0, 2])
def test_c_host_and_device_scalars_hand_the_same_jobs_to_the_device(mods, pairing, extra_aux):
    groth16, _ = mods
    gl = make_gl()
    key = groth16.ResidentProvingKey(gl, pairing, groth16_arrays(pairing), NI)
    inp, aux, h, rs = scalars(NI - 1, 1), scalars(N_AUX + extra_aux, 2), scalars(N_H, 3), scalars(2, 4)
    d_h = gl.DeviceBuffer((N_H + 2) * 96).upload(h)
    got_host = key.create_proof_msms(inp, aux, None, None, rs[0], rs[1], h_dev=(d_h, N_H))
    host, gl.jobs = gl.jobs, []
    d_s = gl.DeviceBuffer((N - 1 + 4) * 96).upload(np.concatenate([inp, aux[:N_AUX]]))       # what gh_r1cs_witness_map_dev leaves: input || aux
    got_dev = key.create_proof_msms(None, None, None, None, rs[0], rs[1], h_dev=(d_h, N_H), scalars_dev=(d_s, N - 1))
    dev = gl.jobs
    one = np.zeros((1, 12), dtype=np.uint64)
    one[0, 0] = 1
    vector = np.concatenate([inp, aux[:N_AUX], one, one, rs]).tobytes()                       # input || aux || 1 || 1 || r || s
    k = key.keys
    tag = lambda name: (k[name].curve, k[name].n, k[name].serial)
    assert [j[0] for j in dev] == [tag(name) for name in ("a", "b1", "h", "l", "b2")]
    assert dev[0][1:] == dev[1][1:] == dev[4][1:] == (N - 1 + 4, vector)
    assert dev[2][1:] == (N_H, h.tobytes()) and dev[3][1:] == (N_AUX, aux[:N_AUX].tobytes())
    if extra_aux == 0:
        assert host == dev
    else:
        # an aux vector longer than the queries: a, b_g1, b_g2 see it cut where the reference's zip cuts it -- the vector the
        # device form holds --, and the l_query's job alone differs: the whole aux vector from an upload of its own
        assert [host[i] for i in (0, 1, 2, 4)] == [dev[i] for i in (0, 1, 2, 4)]
        assert host[3] == (tag("l"), N_AUX + extra_aux, aux.tobytes()) and host[3][2].startswith(dev[3][2])
    for (gxy, ginf), (dxy, dinf) in zip(got_host, got_dev):
        assert ginf == dinf and (gxy == dxy).all()
    assert gl.live_buffers == [d_h, d_s]
    with pytest.raises(ValueError):                                # the device form wants exactly one row per variable and room for four
        key.create_proof_msms(None, None, None, None, rs[0], rs[1], h_dev=(d_h, N_H), scalars_dev=(d_s, N - 2))
    d_small = gl.DeviceBuffer((N - 1 + 3) * 96)
    with pytest.raises(ValueError):
        key.create_proof_msms(None, None, None, None, rs[0], rs[1], h_dev=(d_h, N_H), scalars_dev=(d_small, N - 1))


# ---- (d) a key built from arrays is a whole key
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_d_array_built_key_proves(mods, pairing):
    groth16, _ = mods
    pk = groth16_arrays(pairing)
    blob = groth16_blob(pairing)
    for make in (lambda gl: groth16.ResidentProvingKey(gl, pairing, pk, NI), lambda gl: groth16.ResidentProvingKey.from_parameters(gl, pairing, blob, NI)):
        gl = make_gl()
        key = make(gl)
        assert all(hasattr(key, name) for name in ("gl", "pairing", "num_inputs", "g1", "g2", "keys", "delta_g1"))
        assert (key.gl, key.pairing, key.num_inputs, key.g1, key.g2) == (gl, pairing, NI, pairing + "_g1", pairing + "_g2")
        assert key.delta_g1.dtype == np.uint64 and key.delta_g1.shape == (24,)
        rows = groth16.benchmark_circuit_rows(pairing, N_AUX)
        assert rows[0] == NI and len(rows[1]) == N
        timing = {}
        proof = key.prove_prepared(key.prepare_rows(rows, 1, 2, 3), 4, 5, timing=timing)
        assert len(proof) == 193 + 192 * DEG[pairing + "_g2"] + 1 + 193 and sorted(timing) == ["msm_stage_ms", "rows_upload_ms", "witness_map_ms"]
        assert proof == key.create_proof(rows, 1, 2, 3, 4, 5)
        assert len(gl.jobs) == 10 and gl.live_buffers == [] and gl.live_bases == 5
        key.free()
    assert (groth16.ResidentProvingKey(make_gl(), pairing, pk, NI).delta_g1 == pk["delta_g1"]).all()
