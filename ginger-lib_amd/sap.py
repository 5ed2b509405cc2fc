"""GM17's R1CS -> SAP maps over the resident constraint matrices of r1cs.py (include/ginger_hip_sap.h), with the reference's
names (proof-systems/src/gm17/r1cs_to_sap.rs):

    sap_info(r1cs)                          the SAP domain, the number of SAP variables, the pool bytes of a call
    sap_rows(r1cs, assignment)              the rows witness_map starts its transforms from (:125-189, :206-232) and
                                            full_input_assignment
    sap_rows_dev / sap_witness_map_dev      the same over device buffers, and R1CStoSAP::witness_map as a whole
    sap_instance_map(r1cs, u) / _dev        the loops of instance_map_with_evaluation (:37-94)
    gm17.ResidentGm17Key.create_proof_r1cs / gm17.generate_parameters(..., r1cs=)   the callers above them

Every function takes an r1cs.ResidentR1CS.  Vectors are (n, 12) uint64 Montgomery rows (x 2^768); the scalar destinations
receive canonical limbs.  Everything is exact."""
import ctypes

import numpy as np

from . import _check, _ptr
from . import _handles
from ._handles import _rows, u32, vp


class Info(ctypes.Structure):
    """gh_sap_info_t"""
    _fields_ = [("sap_log_n", u32), ("reserved", u32), ("sap_num_variables", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64)]


_ARGTYPES = {"gh_sap_info": [vp, ctypes.POINTER(Info)],
             "gh_sap_rows_dev": [vp, vp, vp, vp, vp, vp],
             "gh_sap_rows": [vp, vp, vp, vp, vp],
             "gh_sap_r1cs_witness_map_dev": [vp, vp, vp, vp, vp, vp, vp],
             "gh_sap_instance_map_dev": [vp, vp, vp, vp],
             "gh_sap_instance_map": [vp, vp, vp, vp],
             "gh_sap_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_sap.h declares
SAP_SYMBOLS = list(_ARGTYPES)
_lib = _handles.binder("sap", _ARGTYPES)


def _opt(buf):
    return buf.ptr if buf is not None else None


def last_timing(max_phases=40):
    """(device milliseconds per phase of the last call: the conversion or the split, level 0, level 1, ..., the SAP kernel;
    total milliseconds)"""
    return _handles.last_timing(_lib().gh_sap_last_timing, max_phases)


def sap_info(r1cs):
    """-> {"sap_log_n", "size", "sap_num_variables", "scratch_bytes"}; GingerHipError (unsupported) where the SAP domain
    exceeds the field's 2-adicity"""
    out = Info()
    _check(_lib().gh_sap_info(r1cs.handle, ctypes.byref(out)))
    return {"sap_log_n": int(out.sap_log_n), "size": 1 << int(out.sap_log_n), "sap_num_variables": int(out.sap_num_variables),
            "scratch_bytes": int(out.scratch_bytes)}


def sap_rows_dev(r1cs, d_assignment, d_a, d_c, d_scalars=None, d_aux_scalars=None):
    """d_a, d_c: 2^sap_log_n rows; d_scalars: None or sap_num_variables rows; d_aux_scalars: None or sap_num_variables -
    (num_inputs - 1) rows"""
    _check(_lib().gh_sap_rows_dev(r1cs.handle, d_assignment.ptr, d_a.ptr, d_c.ptr, _opt(d_scalars), _opt(d_aux_scalars)))


def sap_rows(r1cs, assignment):
    """-> (full, a, c): full (sap_num_variables + 1, 12), a and c (2^sap_log_n, 12)"""
    z = _rows(assignment)
    if z.shape[0] != r1cs.num_variables:
        raise ValueError("the assignment must have %d rows" % r1cs.num_variables)
    info = sap_info(r1cs)
    a, c = (np.empty((info["size"], 12), dtype=np.uint64) for _ in range(2))
    full = np.empty((info["sap_num_variables"] + 1, 12), dtype=np.uint64)
    _check(_lib().gh_sap_rows(r1cs.handle, _ptr(z), _ptr(a), _ptr(c), _ptr(full)))
    return full, a, c


def sap_witness_map_dev(r1cs, d_assignment, dd, d_h, d_scalars=None, d_aux_scalars=None):
    """dd: (2, 12) Montgomery rows d1, d2; d_h: 2^sap_log_n + 1 rows"""
    dd = _rows(dd)
    _check(_lib().gh_sap_r1cs_witness_map_dev(r1cs.handle, d_assignment.ptr, _ptr(dd[0]), _ptr(dd[1]), d_h.ptr, _opt(d_scalars),
                                              _opt(d_aux_scalars)))


def sap_instance_map_dev(r1cs, d_u, d_a, d_c):
    """d_u: 2^sap_log_n rows; d_a, d_c: sap_num_variables + 1 rows"""
    _check(_lib().gh_sap_instance_map_dev(r1cs.handle, d_u.ptr, d_a.ptr, d_c.ptr))


def sap_instance_map(r1cs, u):
    """u: (2^sap_log_n, 12) -> (a, c), each (sap_num_variables + 1, 12)"""
    u = _rows(u)
    info = sap_info(r1cs)
    if u.shape[0] != info["size"]:
        raise ValueError("u must have %d rows" % info["size"])
    a, c = (np.empty((info["sap_num_variables"] + 1, 12), dtype=np.uint64) for _ in range(2))
    _check(_lib().gh_sap_instance_map(r1cs.handle, _ptr(u), _ptr(a), _ptr(c)))
    return a, c
