/* bmc_abi(): the C ABI of this build of libbmc_hip.so as text, one record per line, made by the compiler from the declarations of
 * include/bmc_hip.h -- the Python binding (bmc_hip/lib.py) builds its argument types, struct mirrors, table dtypes and limits
 * from it.  Host code only; no type, offset or size is written here, only NAMES: the three lists below.
 *   fn     <name> <return code> <parameter code> ...
 *   struct <name> <sizeof> <alignof>
 *   field  <struct> <name> <offset> <size> <element size> <element code> [<extent> [<extent>]]
 *   const  <name> <code> <value>
 * Codes: i4 / u4 / i8 / ... signed / unsigned integer of that many bytes, f4 / f8 float / double, p a pointer (p:<struct> to a
 * bmc_*_t struct, p:char to a C string), s:<struct> a struct by value or as a field.
 * A new entry point, struct, field or numeric #define of the header gets its name added here; tests/test_cabi_and_host.py
 * compares the lists with the header's text, and a field list that does not tile its struct fails the build. */
#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>
#include "bmc_hip.h"
#include "bmc_hip_losses.h"
#include "bmc_hip_quality.h"
#include "bmc_hip_ema.h"
#include "bmc_hip_ssim.h"
#include "bmc_hip_denoise.h"
#include "bmc_hip_downsample.h"
#include "bmc_hip_stream.h"

#define BMC_ABI_FUNCTIONS(X) \
    X(bmc_version) X(bmc_last_error) X(bmc_stream_create_low_priority) X(bmc_events_to_channels) X(bmc_events_binned_ws_bytes) \
    X(bmc_events_to_channels_binned) X(bmc_encode_raw_events_binned) X(bmc_events_torch_ws_ints) X(bmc_events_to_image_torch) \
    X(bmc_events_to_voxel_torch) X(bmc_events_to_voxel) X(bmc_events_to_stack) X(bmc_events_to_stack_polarity) \
    X(bmc_events_to_mask) X(bmc_encode_raw_events) X(bmc_pack_weight) X(bmc_pack_weight_t) X(bmc_split_weight) \
    X(bmc_pack_weight_wino) X(bmc_conv_wino_rows) X(bmc_pack_weight_wino4) X(bmc_conv) X(bmc_pgemm) X(bmc_pgemm_wave_map) \
    X(bmc_pgemm_reduce_weight) X(bmc_pgemm_reduce_weight_groups) X(bmc_pgemm_reduce_plain) X(bmc_wgrad_wino_nsplit) \
    X(bmc_wgrad_wino) X(bmc_wgrad_wino_reduce) X(bmc_wgrad_wino_multi) X(bmc_wgrad_wino4_nsplit) X(bmc_wgrad_wino4) \
    X(bmc_wgrad_wino4_reduce) X(bmc_ptr_table) X(bmc_group_sum) X(bmc_colsum) X(bmc_relu_bwd) X(bmc_layernorm_fwd) \
    X(bmc_layernorm_bwd) X(bmc_softmax_fwd) X(bmc_softmax_bwd) X(bmc_pack_inputs) X(bmc_unshuffle_to_nhwc) X(bmc_shuffle_to_hr) \
    X(bmc_head_mse_fwd) X(bmc_head_mse_bwd) X(bmc_chain_fwd) X(bmc_chain_bwd) X(bmc_chain_affine_grads) X(bmc_small_mm) \
    X(bmc_bicubic_resize_fwd) X(bmc_bicubic_resize_bwd) X(bmc_head_resize_mse_fwd) X(bmc_head_resize_mse_bwd) X(bmc_slot_stage) \
    X(bmc_slot_commit) X(bmc_slot_metrics) X(bmc_slot_encode) X(bmc_seq_encode) X(bmc_seq_encode_crop) X(bmc_slot_emit) \
    X(bmc_slot_emit_timed_scratch_bytes) X(bmc_slot_emit_timed) X(bmc_slot_emit_clocked) X(bmc_slot_hot_update) \
    X(bmc_slot_encode_filtered) X(bmc_hot_pixel_mask) X(bmc_slot_render) X(bmc_slot_voxel) X(bmc_adam_step) \
    X(bmc_adam_step_capturable) X(bmc_adam_grad_sq) X(bmc_adam_step_clipped) X(bmc_adam_step_clipped_capturable)

/* A struct that another one holds by value comes before it. */
#define BMC_ABI_STRUCTS(X) \
    X(bmc_src_t, F(ptr), F(batch_stride), F(pix_stride), F(nch), F(batch_shift), F(batch_mod)) \
    X(bmc_conv_args_t, F(nsrc), F(src), F(wpacked), F(bias), F(w_group_stride), F(bias_group_stride), F(batch_per_group), F(out), \
      F(out_batch_stride), F(out_pix_stride), F(B), F(H), F(W), F(Cout), F(Coutpad), F(taps), F(relu), F(residual), F(mask), \
      F(accumulate), F(math), F(seg_b), F(src_seg_delta), F(residual_seg_delta), F(mask_seg_delta)) \
    X(bmc_pgemm_args_t, F(a), F(nsrc), F(src), F(B), F(H), F(W), F(taps), F(batch_per_group), F(slabs), F(nsplit), F(zeros), \
      F(bias_slabs), F(math), F(tap_groups)) \
    X(bmc_chain_fwd_args_t, F(s0), F(s1), F(wstream), F(bias_f), F(bias_c), F(gamma), F(beta), F(eps), F(yhat), F(rstd), F(centre), \
      F(B), F(C), F(H), F(W)) \
    X(bmc_chain_bwd_args_t, F(dcentre), F(wstream), F(gamma), F(yhat), F(rstd), F(dz), F(ds1), F(ds0), F(ds0_add), F(n), F(C), F(H), \
      F(W)) \
    X(bmc_mm_term_t, F(a), F(a_sb), F(a_sg), F(a_si), F(a_sk), F(b), F(b_sb), F(b_sg), F(b_sk), F(b_sj), F(w), F(w_sb), F(w_sg), \
      F(w_sk)) \
    X(bmc_small_mm_args_t, F(nterms), F(t), F(nbatch), F(batch_per_group), F(M), F(N), F(K), F(alpha), F(u), F(u_sb), F(u_sg), F(v), \
      F(v_sb), F(v_sg), F(c), F(c_sb), F(c_sg), F(c_si), F(c_sj), F(vec_out), F(vo_sb), F(vo_sg), F(accumulate)) \
    X(bmc_slot_t, F(frames), F(gt), F(keep), F(result), F(flags), F(pad_)) \
    X(bmc_slot_events_t, F(lr_xs), F(lr_ys), F(lr_ps), F(gt_xs), F(gt_ys), F(gt_ps), F(gt_range), F(lr_range)) \
    X(bmc_seq_sample_t, F(lr_xs), F(lr_ys), F(lr_ps), F(gt_xs), F(gt_ys), F(gt_ps), F(noise_xs), F(noise_ys), F(noise_ps), \
      F(n_noise), F(flips), F(paused), F(lr_range), F(gt_range)) \
    X(bmc_seq_crop_t, F(H), F(W), F(gh), F(gw), F(top), F(left)) \
    X(bmc_slot_emit_t, F(xs), F(ys), F(ps), F(index_in), F(index_out), F(capacity)) \
    X(bmc_slot_emit_timed_t, F(xs), F(ys), F(ps), F(index_in), F(index_out), F(capacity), F(ts)) \
    X(bmc_slot_clock_t, F(t_first), F(t_last), F(ts)) \
    X(bmc_slot_hot_t, F(hot_pixels), F(hot_mask), F(first_item), F(new_from), F(active), F(pad_), F(cmin)) \
    X(bmc_slot_render_t, F(src), F(dst)) \
    X(bmc_slot_voxel_t, F(dst)) \
    X(bmc_adam_chunk_t, F(p), F(g), F(m), F(v), F(vmax), F(n), F(aligned)) \
    X(bmc_adam_hyper_t, F(lr), F(beta1_f64), F(beta2_f64), F(beta1), F(one_minus_beta1), F(beta2), F(one_minus_beta2), F(eps), \
      F(weight_decay), F(step_size), F(bias_correction2_sqrt), F(amsgrad)) \
    X(bmc_adam_clip_t, F(partial_sq), F(info), F(skipped), F(n_partials), F(max_norm), F(skip_nonfinite))

#define BMC_ABI_CONSTANTS(X) \
    X(BMC_MAX_SRC) X(BMC_CK) X(BMC_SRC_TABLE) X(BMC_MATH_FP32) X(BMC_MATH_BF16) X(BMC_MATH_BF16X6) X(BMC_MATH_FP32_WINO) \
    X(BMC_MATH_FP32_WINO4) X(BMC_MAX_SLOTS) X(BMC_SLOT_ACTIVE) X(BMC_SLOT_RESET) X(BMC_SLOT_MAX_PARTS) X(BMC_SLOT_MAX_SEQN) \
    X(BMC_SEQ_MAX_ITEMS) X(BMC_SLOT_EMIT_MAX_PARTS) X(BMC_EVENT_T0) X(BMC_EVENT_T1) X(BMC_SLOT_EMIT_TIMED_MAX_COUNT) \
    X(BMC_SLOT_EMIT_TIMED_BLOCK) X(BMC_SLOT_EMIT_TIMED_MAX_WINDOW) X(BMC_SLOT_RENDER_MAX_PIXELS) X(BMC_SLOT_RENDER_MAX_PARTS) \
    X(BMC_SLOT_VOXEL_MAX_BINS) X(BMC_ADAM_CHUNK)

/* include/bmc_hip_losses.h, the companion header of the robust-loss head: its own lists and its own text, bmc_losses_abi()
 * (bmc_hip/loss_lib.py binds from it; tests/test_head_loss_cpu.py compares the lists with that header's text). */
#define BMC_LOSSES_ABI_FUNCTIONS(X) X(bmc_head_loss_fwd) X(bmc_head_loss_bwd) X(bmc_losses_abi)
#define BMC_LOSSES_ABI_CONSTANTS(X) X(BMC_LOSS_L1) X(BMC_LOSS_HUBER) X(BMC_LOSS_CHARBONNIER)

/* include/bmc_hip_quality.h, the companion header of the slots' PSNR / SSIM: likewise, bmc_quality_abi() (bmc_hip/quality_lib.py
 * binds from it; tests/test_quality_cpu.py compares the lists with that header's text). */
#define BMC_QUALITY_ABI_FUNCTIONS(X) X(bmc_slot_quality) X(bmc_quality_abi)
#define BMC_QUALITY_ABI_STRUCTS(X) X(bmc_slot_quality_t, F(dst))
#define BMC_QUALITY_ABI_CONSTANTS(X) \
    X(BMC_QUALITY_WIN) X(BMC_QUALITY_WORDS) X(BMC_QUALITY_TILE_H) X(BMC_QUALITY_TILE_W) X(BMC_QUALITY_STATS_WORDS)

/* include/bmc_hip_ema.h, the companion header of the weight EMA inside the optimizer step: likewise, bmc_ema_abi()
 * (bmc_hip/ema_lib.py binds from it; tests/test_optim_ema_cpu.py compares the lists with that header's text). */
#define BMC_EMA_ABI_FUNCTIONS(X) \
    X(bmc_adam_ema_step) X(bmc_adam_ema_step_capturable) X(bmc_adam_ema_step_clipped) X(bmc_adam_ema_step_clipped_capturable) \
    X(bmc_ema_swap) X(bmc_ema_abi)
#define BMC_EMA_ABI_STRUCTS(X) X(bmc_adam_ema_t, F(e), F(decay), F(w), F(warmup))

/* include/bmc_hip_ssim.h, the companion header of the structural training loss: likewise, bmc_ssim_abi() (bmc_hip/ssim_lib.py
 * binds from it; tests/test_ssim_loss_cpu.py compares the lists with that header's text). */
#define BMC_SSIM_ABI_FUNCTIONS(X) X(bmc_ssim_loss_fwd) X(bmc_ssim_loss_bwd) X(bmc_ssim_abi)
#define BMC_SSIM_ABI_CONSTANTS(X) \
    X(BMC_SSIM_WIN) X(BMC_SSIM_TILE_H) X(BMC_SSIM_TILE_W) X(BMC_SSIM_BWD_TILE_H) X(BMC_SSIM_BWD_TILE_W)

/* include/bmc_hip_denoise.h, the companion header of the event noise filter: likewise, bmc_denoise_abi() (bmc_hip/denoise_lib.py
 * binds from it; tests/test_event_denoise_cpu.py compares the lists with that header's text). */
#define BMC_DENOISE_ABI_FUNCTIONS(X) \
    X(bmc_event_denoise_band_rows) X(bmc_event_denoise_scratch_bytes) X(bmc_event_denoise) X(bmc_denoise_abi)
#define BMC_DENOISE_ABI_CONSTANTS(X) X(BMC_DENOISE_STEP) X(BMC_DENOISE_LDS_WORDS) X(BMC_DENOISE_MAX_W)

/* include/bmc_hip_downsample.h, the companion header of the event downsampler: likewise, bmc_downsample_abi()
 * (bmc_hip/downsample_lib.py binds from it; tests/test_event_downsample_cpu.py compares the lists with that header's text). */
#define BMC_DOWNSAMPLE_ABI_FUNCTIONS(X) \
    X(bmc_event_downsample_capacity) X(bmc_event_downsample_chunk) X(bmc_event_downsample_scratch_bytes) \
    X(bmc_event_downsample_keys) X(bmc_event_downsample_walk) X(bmc_event_downsample_gather) X(bmc_downsample_abi)
#define BMC_DOWNSAMPLE_ABI_CONSTANTS(X) \
    X(BMC_DOWNSAMPLE_MAX_SCALE) X(BMC_DOWNSAMPLE_MAX_THRESHOLD) X(BMC_DOWNSAMPLE_LANES) X(BMC_DOWNSAMPLE_TILE) \
    X(BMC_DOWNSAMPLE_MAX_PARTS) X(BMC_DOWNSAMPLE_LAUNCHES)

/* include/bmc_hip_stream.h, the companion header of the continuous (trimmed) event stream: likewise, bmc_stream_abi()
 * (bmc_hip/stream_lib.py binds from it; tests/test_event_stream_cpu.py compares the lists with that header's text). */
#define BMC_STREAM_ABI_FUNCTIONS(X) X(bmc_slot_emit_trimmed) X(bmc_stream_abi)
#define BMC_STREAM_ABI_STRUCTS(X) X(bmc_slot_trim_t, F(t_cut), F(dropped))
#define BMC_STREAM_ABI_CONSTANTS(X) X(BMC_SLOT_TRIM_PARTS)

namespace {

struct field {
    const char* name;
    size_t offset, size, align, elem_size, extent0, extent1;
    std::string (*code)();      /* of the element type */
};
template <class T> struct layout;       /* specialised per listed struct: name, fields */

template <class T> std::string code() {
    if constexpr (std::is_pointer_v<T>) {
        using P = std::remove_cv_t<std::remove_pointer_t<T>>;
        if constexpr (std::is_class_v<P>) return std::string("p:") + layout<P>::name;
        else return std::is_same_v<P, char> ? "p:char" : "p";
    } else if constexpr (std::is_class_v<T>) {
        return std::string("s:") + layout<T>::name;
    } else {
        static_assert(std::is_arithmetic_v<T>, "a type the ABI text has no code for");
        return (std::is_floating_point_v<T> ? "f" : std::is_signed_v<T> ? "i" : "u") + std::to_string(sizeof(T));
    }
}

/* every offset is the previous end rounded up to the field's alignment, and the last end rounded up to the struct's is its size */
template <class T> constexpr bool tiles() {
    size_t end = 0;
    for (const field& f : layout<T>::fields) {
        if (f.offset != (end + f.align - 1) / f.align * f.align) return false;
        end = f.offset + f.size;
    }
    return (end + alignof(T) - 1) / alignof(T) * alignof(T) == sizeof(T);
}

#define F(m) field{#m, offsetof(T, m), sizeof(T::m), alignof(decltype(T::m)), sizeof(std::remove_all_extents_t<decltype(T::m)>), \
                   std::extent_v<decltype(T::m), 0>, std::extent_v<decltype(T::m), 1>, &code<std::remove_all_extents_t<decltype(T::m)>>}
#define BMC_ABI_LAYOUT(S, ...) \
    template <> struct layout<S> { using T = S; static constexpr const char* name = #S; static constexpr field fields[] = {__VA_ARGS__}; }; \
    static_assert(tiles<S>(), #S ": the field list above does not tile the struct (a field is missing or out of order)");
BMC_ABI_STRUCTS(BMC_ABI_LAYOUT)
BMC_QUALITY_ABI_STRUCTS(BMC_ABI_LAYOUT)
BMC_EMA_ABI_STRUCTS(BMC_ABI_LAYOUT)
BMC_STREAM_ABI_STRUCTS(BMC_ABI_LAYOUT)

template <class Fn> struct signature;
template <class R, class... A> struct signature<R (*)(A...)> {
    static std::string text() { return (code<R>() + ... + (" " + code<A>())); }
};

template <class T> void put_struct(std::string& out) {
    const std::string name = layout<T>::name;
    out += "struct " + name + " " + std::to_string(sizeof(T)) + " " + std::to_string(alignof(T)) + "\n";
    for (const field& f : layout<T>::fields) {
        out += "field " + name + " " + f.name + " " + std::to_string(f.offset) + " " + std::to_string(f.size) + " " +
               std::to_string(f.elem_size) + " " + f.code();
        if (f.extent0) out += " " + std::to_string(f.extent0);
        if (f.extent1) out += " " + std::to_string(f.extent1);
        out += "\n";
    }
}

template <class V> std::string number(V v) {
    char buf[40];
    if constexpr (std::is_floating_point_v<V>) snprintf(buf, sizeof buf, "%.17g", (double) v);
    else snprintf(buf, sizeof buf, "%lld", (long long) v);
    return buf;
}

/* <name>(): the text of one header's three lists, made once.  A header without structs or constants passes BMC_ABI_NONE. */
#define BMC_ABI_NONE(X)
#define BMC_ABI_PUT_FN(f) out += "fn " #f " " + signature<decltype(&f)>::text() + "\n";
#define BMC_ABI_PUT_STRUCT(S, ...) put_struct<S>(out);
#define BMC_ABI_PUT_CONST(c) out += "const " #c " " + code<decltype(c)>() + " " + number(c) + "\n";
#define BMC_ABI_TEXT(name, FUNCTIONS, STRUCTS, CONSTANTS)                                   \
    extern "C" const char* name(void) {                                                     \
        static const std::string text = [] {                                                \
            std::string out;                                                                \
            FUNCTIONS(BMC_ABI_PUT_FN) STRUCTS(BMC_ABI_PUT_STRUCT) CONSTANTS(BMC_ABI_PUT_CONST) \
            return out;                                                                     \
        }();                                                                                \
        return text.c_str();                                                                \
    }

}  // namespace

BMC_ABI_TEXT(bmc_abi, BMC_ABI_FUNCTIONS, BMC_ABI_STRUCTS, BMC_ABI_CONSTANTS)
BMC_ABI_TEXT(bmc_losses_abi, BMC_LOSSES_ABI_FUNCTIONS, BMC_ABI_NONE, BMC_LOSSES_ABI_CONSTANTS)
BMC_ABI_TEXT(bmc_quality_abi, BMC_QUALITY_ABI_FUNCTIONS, BMC_QUALITY_ABI_STRUCTS, BMC_QUALITY_ABI_CONSTANTS)
BMC_ABI_TEXT(bmc_ema_abi, BMC_EMA_ABI_FUNCTIONS, BMC_EMA_ABI_STRUCTS, BMC_ABI_NONE)
BMC_ABI_TEXT(bmc_ssim_abi, BMC_SSIM_ABI_FUNCTIONS, BMC_ABI_NONE, BMC_SSIM_ABI_CONSTANTS)
BMC_ABI_TEXT(bmc_denoise_abi, BMC_DENOISE_ABI_FUNCTIONS, BMC_ABI_NONE, BMC_DENOISE_ABI_CONSTANTS)
BMC_ABI_TEXT(bmc_downsample_abi, BMC_DOWNSAMPLE_ABI_FUNCTIONS, BMC_ABI_NONE, BMC_DOWNSAMPLE_ABI_CONSTANTS)
BMC_ABI_TEXT(bmc_stream_abi, BMC_STREAM_ABI_FUNCTIONS, BMC_STREAM_ABI_STRUCTS, BMC_STREAM_ABI_CONSTANTS)
