// The runtime the two codecs share (vae.hip, vqvae.hip): a parameter store on one device with one encode and one decode plan.
// Each fc_vae_* / fc_vqvae_* export forwards to one of these, passing its own name for the error text.
#pragma once
#include <memory>
#include <string>

#include "plan.h"

namespace fc {

struct Codec : ParamStore {
    int device = 0;             // < 0: description only (parameter table, no device memory)
    Plan enc, dec;
    int prec = 0;               // set_precision: arithmetic of the plans built from now on (0 exact fp32, 1 split-bf16)
    int taps = 0;               // debug_taps: the plans built from now on recycle no buffer and name their tensors (PlanBuilder::keep_all)
    const Plan& plan(int decode) const { return decode ? dec : enc; }
};

inline int codec_fail(int code, const char* fn, const char* what) { return fail(code, std::string(fn) + ": " + what); }

// `declare` fills the parameter table of `v`; on a device >= 0 the weights are then allocated there, the packed copy zeroed (padded
// slots stay zero beyond every load).
template <class T>
int codec_create(std::unique_ptr<T> v, int device, int (*declare)(T*), T** out) {
    v->device = device;
    v->want_b3 = device >= 0;      // the split-bf16 copies of the conv weights (set_precision): +1x the conv weights in HBM
    FC_TRY(declare(v.get()));
    if (device >= 0) {
        FC_TRY(fc_check_device(device));
        FC_HIP(hipSetDevice(device));
        FC_TRY(conv_init());
        FC_TRY(v->alloc_device());
        FC_HIP(hipMemset(v->packed, 0, (size_t)(v->packed_numel ? v->packed_numel : 4) * sizeof(float)));
    }
    *out = v.release();
    return FC_OK;
}

template <class T>
void codec_destroy(T* v) {
    if (!v) return;
    if (v->device >= 0) {
        (void)hipSetDevice(v->device);
        (void)hipDeviceSynchronize();
        v->enc.release();
        v->dec.release();
        v->free_device();
    }
    delete v;
}

inline int codec_load(Codec* v, const char* fn, const float* flat, int64_t numel, int on_device, void* stream) {
    if (!v || !flat) return codec_fail(FC_E_ARG, fn, "null argument");
    if (v->device < 0) return codec_fail(FC_E_STATE, fn, "created with device < 0 (description only)");
    FC_HIP(hipSetDevice(v->device));
    return v->load(flat, numel, on_device, static_cast<hipStream_t>(stream));
}

// A switch the builders read has changed: the plans in place were built the other way and are dropped, the next reserve rebuilds.
inline int codec_drop_plans(Codec* v) {
    if (v->device < 0) return FC_OK;
    FC_HIP(hipSetDevice(v->device));
    FC_HIP(hipDeviceSynchronize());
    v->enc.release(); v->dec.release();
    return FC_OK;
}

inline int codec_set_precision(Codec* v, const char* fn, int mode) {
    if (!v || (mode != 0 && mode != 1)) return codec_fail(FC_E_ARG, fn, "mode is 0 (fp32) or 1 (split-bf16)");
    if (v->prec == mode) return FC_OK;
    v->prec = mode;
    return codec_drop_plans(v);
}

// Debug taps (tests only): plans that recycle no buffer and name their tensors (PlanBuilder::keep_all).
inline int codec_debug_taps(Codec* v, const char* fn, int on) {
    if (!v) return codec_fail(FC_E_ARG, fn, "null handle");
    on = on ? 1 : 0;
    if (v->taps == on) return FC_OK;
    v->taps = on;
    return codec_drop_plans(v);
}

// A tensor the encode / decode plan recorded under `name` (NHWC, plan.maxB rows); only plans built with taps on have any.
inline int codec_debug_tensor(const Codec* v, const char* fn, int decode, const char* name, const float** ptr, int* C, int* H, int* W) {
    if (!v || !name || !ptr || !C || !H || !W) return codec_fail(FC_E_ARG, fn, "null argument");
    const Plan& pl = v->plan(decode);
    auto it = pl.named.find(name);
    if (it == pl.named.end()) return codec_fail(FC_E_ARG, fn, (std::string("no tap named ") + name + (v->taps ? "" : " (debug taps are off)")).c_str());
    *ptr = it->second.p; *C = it->second.C; *H = it->second.H; *W = it->second.W;
    return FC_OK;
}

// Builds the encode (decode) plan with `build` unless the one in place covers max_batch rows at this shape.
template <class T>
int codec_reserve(T* v, const char* fn, int decode, int (*build)(T*, int, int, int), int max_batch, int height, int width) {
    if (!v || max_batch < 1 || v->device < 0) return codec_fail(FC_E_ARG, fn, "bad argument");
    Plan& pl = decode ? v->dec : v->enc;
    if (pl.maxB >= max_batch && pl.H == height && pl.W == width) return FC_OK;
    FC_HIP(hipSetDevice(v->device));
    FC_HIP(hipDeviceSynchronize());
    const int r = build(v, max_batch, height, width);
    if (r != FC_OK) pl.release();
    return r;
}

inline int codec_run(const Codec* v, const char* fn, int decode, const float* in, float* out, int B, int H, int W, void* stream) {
    if (!v || !in || !out || B < 1) return codec_fail(FC_E_ARG, fn, "null argument");
    if (!v->loaded) return codec_fail(FC_E_STATE, fn, "weights not loaded (load_params)");
    const Plan& pl = v->plan(decode);
    if (pl.maxB < B || pl.H != H || pl.W != W) return codec_fail(FC_E_STATE, fn, "no plan for this shape; reserve it first");
    FwdCtx c;
    c.x = in; c.x_mod = B; c.out = out; c.B = B;
    return run_plan(pl, c, static_cast<hipStream_t>(stream));
}

// The record of launch i of a plan; null outputs are skipped.
inline int codec_op_info(const Codec* v, const char* fn, int decode, int i, const char** kernel, const char** module, double* flops_per_sample,
                         double* bytes_per_sample, double* bytes_per_launch) {
    if (!v) return codec_fail(FC_E_ARG, fn, "null handle");
    const Plan& pl = v->plan(decode);
    if (i < 0 || i >= (int)pl.ops.size()) return codec_fail(FC_E_ARG, fn, "index out of range");
    if (kernel) *kernel = pl.op_kernel[i].c_str();
    if (module) *module = pl.op_what[i].c_str();
    if (flops_per_sample) *flops_per_sample = pl.op_flops[i];
    if (bytes_per_sample) *bytes_per_sample = pl.op_bytes_ps[i];
    if (bytes_per_launch) *bytes_per_launch = pl.op_bytes_fixed[i];
    return FC_OK;
}

// Measurement hook: every launch of the encode / decode plan timed alone (profile_plan).  in_dev / out_dev: valid input and output
// tensors for `batch` samples at the plan's shape.  Synchronises.
inline int codec_profile(const Codec* v, const char* fn, int decode, const float* in_dev, float* out_dev, int batch, int repeats, float* ms_out,
                         int n_out, void* stream) {
    if (!v || !in_dev || !out_dev || !ms_out || repeats < 1) return codec_fail(FC_E_ARG, fn, "bad argument");
    const Plan& pl = v->plan(decode);
    if (pl.maxB < batch || pl.ops.empty()) return codec_fail(FC_E_STATE, fn, "reserve the plan first");
    if (!v->loaded) return codec_fail(FC_E_STATE, fn, "weights not loaded (load_params)");
    FwdCtx c;
    c.x = in_dev; c.x_mod = batch; c.out = out_dev; c.B = batch;
    return profile_plan(pl, c, repeats, ms_out, n_out, static_cast<hipStream_t>(stream));
}

}  // namespace fc
