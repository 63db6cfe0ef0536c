// Weight re-layout from the reference's state_dict tensors to the kernels' operand layouts.  Runs once per
// fc_unet_load_params (and once per optimiser step when training), HBM-bound and tiny.
//
// The layouts are the PackKinds of common.h, where each is documented beside its name: PACK_CONV, PACK_S2D, PACK_TRANSPOSE, PACK_COPY,
// PACK_CONV_PAD, PACK_DGRAD, PACK_CONV_K8, PACK_CONV_B3, PACK_UP4, PACK_UP4_B3.  One kernel runs a whole table of such jobs in ONE launch
// (a training step re-packs ~190 weight tensors: launch latency, not bytes); there is no other packer.
#include <vector>

#include "common.h"

namespace fc {

// element (o, ci, tap) of an OIHW tensor with I input channels and KK taps
__device__ __forceinline__ size_t oihw(int o, int ci, int tap, int I, int KK) { return ((size_t)o * I + ci) * KK + tap; }

// t over [n2][n1][n0], n0 fastest
__device__ __forceinline__ void unflatten(size_t t, int n0, int n1, int& i0, int& i1, int& i2) {
    i0 = (int)(t % n0);
    const size_t r = t / n0;
    i1 = (int)(r % n1); i2 = (int)(r / n1);
}
// t over [tap][Ipad/8][O][8] (the split-bf16 layouts) -> o, ci = 8 c8 + jj, tap
__device__ __forceinline__ void unflatten_oct(size_t t, int O, int Ipad, int& o, int& ci, int& tap) {
    const int jj = (int)(t & 7);
    int c8;
    unflatten(t >> 3, O, Ipad / 8, o, c8, tap);
    ci = 8 * c8 + jj;
}

// x = hi + lo as bf16: hi = bf16(x) to nearest even, lo = bf16(x - hi)
__device__ __forceinline__ unsigned short bf16_rne(float x) {
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ __forceinline__ void split_bf16(float x, unsigned short* hi, unsigned short* lo) {
    *hi = bf16_rne(x);
    *lo = bf16_rne(x - __uint_as_float((unsigned)*hi << 16));
}

// PACK_UP4 / PACK_UP4_B3: the sum of the 3x3 taps of w(o, ci, .) that land on tap (ty, tx) of the 2x2 kernel of parity (pa, pb)
__device__ __forceinline__ float fold_up4(const float* w, int par, int tap) {
    const int pa = par >> 1, pb = par & 1, ty = tap >> 1, tx = tap & 1;
    const int ky0 = pa == 0 ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), ky1 = pa == 0 ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
    const int kx0 = pb == 0 ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kx1 = pb == 0 ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
    float x = 0.f;
    for (int ky = ky0; ky <= ky1; ++ky)
        for (int kx = kx0; kx <= kx1; ++kx) x += w[ky * 3 + kx];
    return x;
}

__global__ void __launch_bounds__(256) pack_table_kernel(const PackJob* jobs, const int2* blocks) {
    const int2 bj = blocks[blockIdx.x];          // (job, block index inside the job)
    const PackJob j = jobs[bj.x];
    const float* src = j.src;
    float* dst = j.dst;
    unsigned short* d16 = reinterpret_cast<unsigned short*>(dst);
    const size_t lo = (size_t)bj.y * kPackPerBlock, hi = lo + kPackPerBlock < j.total ? lo + kPackPerBlock : j.total;
    for (size_t t = lo + threadIdx.x; t < hi; t += 256) {
        int o, ci, tap;
        switch (j.kind) {
            case PACK_CONV:
                unflatten(t, j.a, j.b, o, ci, tap);
                dst[t] = src[oihw(o, ci, tap, j.b, j.c)];
                break;
            case PACK_S2D:
                unflatten(t, j.a, j.b, o, ci, tap);
                dst[t] = src[oihw(o, ci, tap, j.b, 4)];
                break;
            case PACK_TRANSPOSE: {
                const int r = (int)(t % j.a), c = (int)(t / j.a);
                dst[(size_t)c * j.c + j.d + r] = src[(size_t)r * j.b + c];
                break; }
            case PACK_COPY:
                dst[t] = src[t];
                break;
            case PACK_CONV_PAD:
                unflatten(t, j.d, j.e, o, ci, tap);
                dst[t] = (o < j.a && ci < j.b) ? src[oihw(o, ci, tap, j.b, j.c)] : 0.f;
                break;
            case PACK_DGRAD: {
                int i;
                unflatten(t, j.e, j.a, i, o, tap);
                const int ky = j.c - 1 - tap / j.c, kx = j.c - 1 - tap % j.c;
                dst[t] = src[oihw(o, j.d + i, ky * j.c + kx, j.b, j.c * j.c)];
                break; }
            case PACK_CONV_K8: {
                const int jj = (int)(t & 3);
                size_t r = t >> 2;
                o = (int)(r % j.a); r /= j.a;
                const int half = (int)(r & 1); r >>= 1;
                const int c8 = (int)(r % (j.b / 8));
                tap = (int)(r / (j.b / 8));
                dst[t] = src[oihw(o, 8 * c8 + 2 * jj + half, tap, j.b, j.c)];
                break; }
            case PACK_CONV_B3:
                unflatten_oct(t, j.a, j.d, o, ci, tap);
                split_bf16(ci < j.b ? src[oihw(o, ci, tap, j.b, j.c)] : 0.f, d16 + t, d16 + j.total + t);
                break;
            case PACK_UP4: {
                const size_t per = (size_t)4 * j.b * j.a;      // elements of one parity
                const int par = (int)(t / per);
                unflatten(t - par * per, j.a, j.b, o, ci, tap);
                dst[t] = fold_up4(src + oihw(o, ci, 0, j.b, 9), par, tap);
                break; }
            case PACK_UP4_B3: {
                const size_t per = (size_t)4 * j.c * j.a;      // elements of one part of one parity
                const int par = (int)(t / per);
                const size_t e = t - par * per;
                unflatten_oct(e, j.a, j.c, o, ci, tap);
                unsigned short* d = d16 + (size_t)par * 2 * per + e;
                split_bf16(ci < j.b ? fold_up4(src + oihw(o, ci, 0, j.b, 9), par, tap) : 0.f, d, d + per);
                break; }
            case PACK_KINDS: break;     // not a layout: pack_table_build lets none through
        }
    }
}

int pack_table_build(const std::vector<PackJob>& jobs, PackTable* out) {
    out->release();
    std::vector<int2> blocks;
    for (size_t i = 0; i < jobs.size(); ++i) {
        if (jobs[i].kind < 0 || jobs[i].kind >= PACK_KINDS) return fail(FC_E_ARG, "pack: job " + std::to_string(i) + " names no layout (kind " + std::to_string((int)jobs[i].kind) + ")");
        const int nb = (int)((jobs[i].total + kPackPerBlock - 1) / kPackPerBlock);
        for (int b = 0; b < nb; ++b) blocks.push_back(make_int2((int)i, b));
    }
    if (blocks.empty()) return FC_OK;
    FC_TRY(dev_alloc(reinterpret_cast<void**>(&out->jobs), jobs.size() * sizeof(PackJob), "pack.jobs"));
    FC_TRY(dev_alloc(reinterpret_cast<void**>(&out->blocks), blocks.size() * sizeof(int2), "pack.blocks"));
    FC_HIP(hipMemcpy(out->jobs, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
    FC_HIP(hipMemcpy(out->blocks, blocks.data(), blocks.size() * sizeof(int2), hipMemcpyHostToDevice));
    out->nblocks = (int)blocks.size();
    return FC_OK;
}

void PackTable::release() {
    if (jobs) dev_free(jobs);
    if (blocks) dev_free(blocks);
    jobs = nullptr; blocks = nullptr; nblocks = 0;
}

int pack_table_launch(const PackTable& t, hipStream_t s) {
    if (!t.nblocks) return FC_OK;
    hipLaunchKernelGGL(pack_table_kernel, dim3(t.nblocks), dim3(256), 0, s, t.jobs, t.blocks);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// [B][R][Cc] -> [B][Cc][R] through a padded 32x32 LDS tile (coalesced on both sides).   grid (Cc/32, R/32, B), block (32, 8)
__global__ void __launch_bounds__(256) transpose_batched_kernel(const float* src, float* dst, int R, int Cc) {
    __shared__ float tile[32][33];
    const size_t base = (size_t)blockIdx.z * R * Cc;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8)
        if (r0 + j < R && c0 + threadIdx.x < Cc) tile[j][threadIdx.x] = src[base + (size_t)(r0 + j) * Cc + c0 + threadIdx.x];
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8)
        if (c0 + j < Cc && r0 + threadIdx.x < R) dst[base + (size_t)(c0 + j) * R + r0 + threadIdx.x] = tile[threadIdx.x][j];
}

int transpose_batched_launch(const float* src, float* dst, int B, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(transpose_batched_kernel, dim3(cdiv(cols, 32), cdiv(rows, 32), B), dim3(32, 8), 0, s, src, dst, rows, cols);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // namespace fc
