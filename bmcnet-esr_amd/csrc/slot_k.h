// Accessors shared by the slot and event kernels (internal): slots.hip, slot_encode_k.h and wave_k.h (and through it
// slot_emit_k.h, ssim_k.h, slot_hot.hip, slot_render.hip, event_denoise.hip, event_downsample.hip, scatter.hip).  Pointers read from a slot
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
