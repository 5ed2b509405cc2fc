// The pairing kernels and host steps instantiated for MNT6-753 (see pairing_impl.h, pairing29_mnt6.h); the C ABI is pairing.hip.
#include "pairing_impl.h"
#include "gm17_verify_impl.h"
GH_DEFINE_PAIRING_OPS(gh::Mnt6Pairing, pairing_ops_mnt6753)
