"""What the Groth16 and GM17 provers (groth16.py, gm17.py) share above the C ABI: the resident query set of a proving key
and three small helpers for device vectors of 96-byte rows."""
import ctypes

import numpy as np


class RowView:
    """the rows of a DeviceBuffer from row0 on, where a call takes something with a .ptr"""

    def __init__(self, buf, row0):
        self.ptr = ctypes.c_void_p(buf.ptr.value + row0 * 96)


def upload_rows(gl, buf, parts, row0=0):
    """(n, 12) u64 host arrays back to back into buf's rows from row0 on -> the row behind the last one written
    (piecewise: concatenating 100 MB host vectors first costs more than the MSM stage's sort)"""
    lib = gl.load_library()
    for part in parts:
        if len(part):
            part = np.ascontiguousarray(part, dtype=np.uint64)
            assert row0 * 96 + part.nbytes <= buf.nbytes
            gl._check(lib.gh_dev_upload(RowView(buf, row0).ptr, gl._ptr(part), part.nbytes))
            row0 += len(part)
    return row0


def into_repr(gl, field, buf, rows):
    """the first `rows` Montgomery rows of buf -> canonical scalars, in place on the device"""
    one_plain = np.zeros(12, dtype=np.uint64)
    one_plain[0] = 1
    gl._check(gl.load_library().gh_vec_scale_dev(gl.FIELDS[field], buf.ptr, gl._ptr(one_plain), rows))


class ResidentQueries:
    """The query vectors of one proving key on the device: keys[name] is a ResidentBases."""

    def __init__(self, gl, pairing, num_inputs):
        assert pairing in ("mnt4753", "mnt6753")
        self.gl, self.pairing, self.num_inputs = gl, pairing, int(num_inputs)
        self.g1, self.g2 = pairing + "_g1", pairing + "_g2"
        self.keys = {}

    def _upload(self, vectors, precompute):
        """vectors: name -> (curve, GroupAffine::write records as bytes) or (curve, Montgomery x || y rows, infinity flags or
        None).  Nothing stays on the device if one of the uploads fails."""
        gl = self.gl
        try:
            for name, (curve, data, *inf) in vectors.items():
                wire = isinstance(data, (bytes, bytearray))
                rb = self.keys[name] = gl.ResidentBases.from_wire(curve, data) if wire else gl.ResidentBases(curve, data, infinity=inf[0])
                if precompute and rb.n:
                    try:
                        rb.precompute(0)
                    except gl.GingerHipError:
                        pass                  # no memory for the table / a point of 2-power order: per-window path
        except BaseException:
            self.free()
            raise

    def free(self):
        for rb in self.keys.values():
            rb.free()

    close = free

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
