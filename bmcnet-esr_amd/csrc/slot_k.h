// Accessors shared by the slot kernels (internal): slots.hip, slot_encode_k.h and slot_emit_k.h.  Pointers read from a slot
// table are generic to the compiler; every access through them goes through an address-space(1) cast (global_* instructions,
// never flat_*).
#pragma once
#include "bmc_common.h"

namespace {

template <class T>
__device__ __forceinline__ T gld(const void* p) {
    return *(const __attribute__((address_space(1))) T*)(unsigned long long)p;
}
template <class T>
__device__ __forceinline__ void gst(void* p, T v) {
    *(__attribute__((address_space(1))) T*)(unsigned long long)p = v;
}

}  // namespace
