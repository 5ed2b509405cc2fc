// Host-side shim over ginger-lib_amd/csrc/sap_rows.h for tests/test_sap_host.py: the lanes of the SAP kernels run in a loop
// over the products of r1cs_plan.h's host executor (sap_host.h), compiled by g++ (no GPU, no HIP).
// Build: g++ -O2 -std=c++17 -shared -fPIC -o build/libsap_shim.so tests/host_shim/sap_shim.cpp.  Test infrastructure.
#include "sap_host.h"

using namespace gh;

namespace {

bool valid(uint64_t ni, uint64_t na, uint64_t nc, const gh_r1cs_matrix_t* m) {
    if (!ni) return false;
    for (int k = 0; k < 3; k++)
        if (r1cs_check_csr(nc, ni + na, m[k].row_ptr, m[k].col, m[k].coeff_id, m[k].num_coeffs)) return false;
    return true;
}

template <class P>
int rows(uint64_t ni, uint64_t na, uint64_t nc, const gh_r1cs_matrix_t* m, uint32_t S, const uint64_t* z, uint64_t* a, uint64_t* c, uint64_t* scalars,
         uint64_t* aux, uint64_t* full) {
    SapShape sh;
    uint32_t log_n;
    if (!sap_host::shape<P>(ni, na, nc, sh, &log_n)) return -2;
    sap_host::rows<P>(sh, m, S, z, a, c, scalars, aux, full);
    return 0;
}

template <class P> int instance_map(uint64_t ni, uint64_t na, uint64_t nc, const gh_r1cs_matrix_t* m, uint32_t S, const uint64_t* u, uint64_t* a, uint64_t* c) {
    SapShape sh;
    uint32_t log_n;
    if (!sap_host::shape<P>(ni, na, nc, sh, &log_n)) return -2;
    sap_host::instance_map<P>(sh, m, S, u, a, c);
    return 0;
}

}  // namespace

extern "C" {

// field: 0 = MNT4-753 Fr (P6), 1 = MNT6-753 Fr (P4), the ids of gh_field_t.  0, or -2 (GH_E_UNSUPPORTED) where the SAP domain
// exceeds the field's 2-adicity
int sap_shim_info(int field, uint64_t ni, uint64_t na, uint64_t nc, uint32_t* log_n, uint64_t* sap_nv, uint64_t* lanes) {
    SapShape sh;
    if (!(field == 0 ? sap_host::shape<P6>(ni, na, nc, sh, log_n) : sap_host::shape<P4>(ni, na, nc, sh, log_n))) return -2;
    *sap_nv = sh.sap_nv();
    *lanes = sh.rows_lanes();
    return 0;
}

int sap_shim_rows(int field, uint64_t ni, uint64_t na, uint64_t nc, const gh_r1cs_matrix_t* m, uint32_t S, const uint64_t* z, uint64_t* a, uint64_t* c,
                  uint64_t* scalars, uint64_t* aux, uint64_t* full) {
    if (!valid(ni, na, nc, m)) return -1;
    return field == 0 ? rows<P6>(ni, na, nc, m, S, z, a, c, scalars, aux, full) : rows<P4>(ni, na, nc, m, S, z, a, c, scalars, aux, full);
}

int sap_shim_instance_map(int field, uint64_t ni, uint64_t na, uint64_t nc, const gh_r1cs_matrix_t* m, uint32_t S, const uint64_t* u, uint64_t* a,
                          uint64_t* c) {
    if (!valid(ni, na, nc, m)) return -1;
    return field == 0 ? instance_map<P6>(ni, na, nc, m, S, u, a, c) : instance_map<P4>(ni, na, nc, m, S, u, a, c);
}

}  // extern "C"
