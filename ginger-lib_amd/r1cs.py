"""The constraint matrices of an R1CS instance resident on the device (include/ginger_hip_r1cs.h) and the sparse products
over them, with the reference's names (proof-systems/src/groth16/r1cs_to_qap.rs):

    ResidentR1CS(gl, pairing, lcs)        upload of at / bt / ct, once per circuit
      .evaluate(assignment)               the rows a, b, c witness_map forms (:78-119, :141-151), padded to the QAP domain
      .instance_map(u)                    the loops of instance_map_with_evaluation (:32-65)
      .matvec(which, x, transpose)        y = M x or M^T x for M = A, B, C
      .info()                             sizes, the schedule's shape, the dictionary's classes, device bytes
    groth16.ResidentProvingKey.create_proof_r1cs / groth16.generate_parameters(..., r1cs=)   the callers above them

`lcs` is (num_inputs, num_aux, at, bt, ct) as groth16.benchmark_circuit_lcs returns it: rows of (coefficient, index) with
integer coefficients and index 0 the constant one -- what KeypairAssembly / ProvingAssignment hold after synthesis.  Vectors
are (n, 12) uint64 Montgomery rows (x 2^768).  Everything is exact."""
import ctypes

import numpy as np

from . import FIELDS, DeviceBuffer, GingerHipError, _check, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles
from .limbs import FR_FIELD, MODULUS, mont_rows
from ._handles import _rows, ci, sz, u32, vp

MATRICES = ("A", "B", "C")
CLASSES = ("zero", "one", "minus_one", "small", "minus_small", "general")


class Matrix(ctypes.Structure):
    """gh_r1cs_matrix_t"""
    _fields_ = [("row_ptr", vp), ("col", vp), ("coeff_id", vp), ("coeff_values", vp), ("num_coeffs", sz)]


class Info(ctypes.Structure):
    """gh_r1cs_info_t"""
    _fields_ = [("num_inputs", ctypes.c_uint64), ("num_aux", ctypes.c_uint64), ("num_constraints", ctypes.c_uint64),
                ("log_n", u32), ("segment_terms", u32), ("nnz", ctypes.c_uint64 * 2 * 3), ("longest_row", u32 * 2 * 3),
                ("levels", u32 * 2 * 3), ("class_counts", u32 * 6), ("device_bytes", ctypes.c_uint64)]


_ARGTYPES = {"gh_r1cs_upload": [ci, sz, sz, sz, ctypes.POINTER(Matrix), u32, _handles.OUT_HANDLE],
             "gh_r1cs_free": [vp],
             "gh_r1cs_info": [vp, ctypes.POINTER(Info)],
             "gh_r1cs_matvec_dev": [vp, ci, ci, vp, vp],
             "gh_r1cs_evaluate_dev": [vp, vp, vp, vp, vp],
             "gh_r1cs_evaluate": [vp, vp, vp, vp, vp],
             "gh_r1cs_witness_map_dev": [vp, vp, vp, vp, vp, vp, vp],
             "gh_r1cs_instance_map_dev": [vp, vp, vp, vp, vp],
             "gh_r1cs_instance_map": [vp, vp, vp, vp, vp],
             "gh_r1cs_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_r1cs.h declares
R1CS_SYMBOLS = list(_ARGTYPES)
_lib = _handles.binder("r1cs", _ARGTYPES)


def flatten(rows, modulus):
    """rows of (coefficient, index) -> the CSR arrays and the dictionary of the C ABI:
    (row_ptr (n + 1,) uint64, col (nnz,) uint32, coeff_id (nnz,) uint32, coeff_values (num_coeffs, 12) uint64 Montgomery).
    Coefficients are integers, taken modulo the field; equal values share one dictionary entry."""
    row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
    ids, cols, values = [], [], {}
    for i, row in enumerate(rows):
        for cf, ix in row:
            cols.append(ix)
            ids.append(values.setdefault(int(cf) % modulus, len(values)))
        row_ptr[i + 1] = len(cols)
    return row_ptr, np.array(cols, dtype=np.uint32), np.array(ids, dtype=np.uint32), mont_rows(values, modulus)     # in order of first use


def last_timing(max_phases=40):
    """(device milliseconds per phase of the last call: input conversion, level 0, level 1, ..., what follows the products;
    total milliseconds)"""
    return _handles.last_timing(_lib().gh_r1cs_last_timing, max_phases)


class ResidentR1CS:
    """A, B, C of one circuit on the device, in both orientations.  segment_terms: 0 = the library's default."""

    def __init__(self, gl, pairing, lcs, segment_terms=0):
        num_inputs, num_aux, at, bt, ct = lcs
        if len(bt) != len(at) or len(ct) != len(at):
            raise ValueError("at, bt and ct must have one row per constraint")
        self._init(gl, pairing, num_inputs, num_aux, len(at), [flatten(rows, MODULUS[pairing]) for rows in (at, bt, ct)], segment_terms)

    def _init(self, gl, pairing, num_inputs, num_aux, num_constraints, arrays, segment_terms):
        """arrays: three (row_ptr, col, coeff_id, coeff_values) tuples of contiguous arrays, alive across the call"""
        self.gl, self.pairing = gl, pairing
        self.field, self.modulus = FIELDS[FR_FIELD[pairing]], MODULUS[pairing]
        self.num_inputs, self.num_aux, self.num_constraints = int(num_inputs), int(num_aux), int(num_constraints)
        self.num_variables = self.num_inputs + self.num_aux
        self.handle = None
        ms = (Matrix * 3)()
        for m, (row_ptr, col, ids, vals) in zip(ms, arrays):
            m.row_ptr, m.col, m.coeff_id, m.coeff_values, m.num_coeffs = _ptr(row_ptr), _ptr(col), _ptr(ids), _ptr(vals), len(vals)
        h = vp()
        _check(_lib().gh_r1cs_upload(self.field, self.num_inputs, self.num_aux, self.num_constraints, ms, segment_terms, ctypes.byref(h)))
        self.handle = h
        self.log_n = self.info()["log_n"]
        self.size = 1 << self.log_n

    @classmethod
    def from_csr(cls, gl, pairing, num_inputs, num_aux, num_constraints, matrices, segment_terms=0):
        """the same from three (row_ptr, col, coeff_id, coeff_values) tuples in the C ABI's form"""
        self = cls.__new__(cls)
        keep = [(np.ascontiguousarray(p, dtype=np.uint64), np.ascontiguousarray(c, dtype=np.uint32), np.ascontiguousarray(k, dtype=np.uint32),
                 np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 12)) for p, c, k, v in matrices]
        self._init(gl, pairing, num_inputs, num_aux, num_constraints, keep, segment_terms)
        return self

    def free(self):
        if self.handle:
            _lib().gh_r1cs_free(self.handle)
            self.handle = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def info(self):
        out = Info()
        _check(_lib().gh_r1cs_info(self.handle, ctypes.byref(out)))
        per = lambda f: {m: (int(f[k][0]), int(f[k][1])) for k, m in enumerate(MATRICES)}   # (M, M^T)
        return {"num_inputs": int(out.num_inputs), "num_aux": int(out.num_aux), "num_constraints": int(out.num_constraints),
                "log_n": int(out.log_n), "segment_terms": int(out.segment_terms), "nnz": per(out.nnz), "longest_row": per(out.longest_row),
                "levels": per(out.levels), "class_counts": dict(zip(CLASSES, (int(c) for c in out.class_counts))),
                "device_bytes": int(out.device_bytes)}

    def _which(self, which):
        return MATRICES.index(which) if isinstance(which, str) else int(which)

    def matvec_dev(self, which, d_x, d_y, transpose=False):
        """device pointers (DeviceBuffer): y = M x, or M^T x"""
        _check(_lib().gh_r1cs_matvec_dev(self.handle, self._which(which), int(bool(transpose)), d_x.ptr, d_y.ptr))

    def matvec(self, which, x, transpose=False):
        n_in, n_out = (self.num_constraints, self.num_variables) if transpose else (self.num_variables, self.num_constraints)
        x = _rows(x)
        if x.shape[0] != n_in:
            raise ValueError("x must have %d rows" % n_in)
        d_x, d_y = DeviceBuffer(max(96, n_in * 96)), DeviceBuffer(max(96, n_out * 96))
        try:
            d_x.upload(x)
            self.matvec_dev(which, d_x, d_y, transpose)
            return d_y.download()[:n_out * 12].reshape(n_out, 12)
        finally:
            d_x.free()
            d_y.free()

    def evaluate(self, assignment):
        """-> (a, b, c), each (2^log_n, 12): A z, B z, C z, then a's input rows (one, z_1 ...), then zeros"""
        z = _rows(assignment)
        if z.shape[0] != self.num_variables:
            raise ValueError("the assignment must have %d rows" % self.num_variables)
        out = [np.empty((self.size, 12), dtype=np.uint64) for _ in range(3)]
        _check(_lib().gh_r1cs_evaluate(self.handle, _ptr(z), *(_ptr(o) for o in out)))
        return tuple(out)

    def evaluate_dev(self, d_assignment, d_a, d_b, d_c):
        _check(_lib().gh_r1cs_evaluate_dev(self.handle, d_assignment.ptr, d_a.ptr, d_b.ptr, d_c.ptr))

    def witness_map_dev(self, d_assignment, dd, d_h, d_scalars=None):
        """dd: (3, 12) Montgomery rows d1, d2, d3; d_h: 2^log_n + 1 rows; d_scalars: None or num_variables - 1 rows"""
        dd = _rows(dd)
        _check(_lib().gh_r1cs_witness_map_dev(self.handle, d_assignment.ptr, _ptr(dd[0]), _ptr(dd[1]), _ptr(dd[2]), d_h.ptr,
                                              d_scalars.ptr if d_scalars is not None else None))

    def instance_map(self, u):
        """u: (2^log_n, 12) -> (a, b, c), each (num_variables, 12)"""
        u = _rows(u)
        if u.shape[0] != self.size:
            raise ValueError("u must have %d rows" % self.size)
        out = [np.empty((self.num_variables, 12), dtype=np.uint64) for _ in range(3)]
        _check(_lib().gh_r1cs_instance_map(self.handle, _ptr(u), *(_ptr(o) for o in out)))
        return tuple(out)

    def instance_map_dev(self, d_u, d_a, d_b, d_c):
        _check(_lib().gh_r1cs_instance_map_dev(self.handle, d_u.ptr, d_a.ptr, d_b.ptr, d_c.ptr))
