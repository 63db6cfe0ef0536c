// Residual(PreNorm(LinearAttention)) (unet.py:125-161) without ever materialising q, k, v or the attention output:
//
//   la_ctx    grid (heads, B): k, v = GroupNorm(x) . Wk, Wv on the matrix pipe, 32 positions at a time per wave, fed straight into
//             an ONLINE softmax over the positions (running column maximum, rescaled accumulators) and the 32x32 context
//             ctx[d][e] = sum_n softmax_n(k)[d][n] v[e][n], itself an MFMA over the positions.  The four waves' partial
//             (max, sum, context) triples are merged at the end.  Traffic: x once per head, the context out.
//   la_apply  grid (ceil(n/128), B): q = GroupNorm(x) . Wq, softmax over the head dimension by lane shuffles, out = q . ctx,
//             y = out . Wout + b, all per 32-row tile per wave with the operands handed between the three GEMMs through a
//             4 KB LDS tile; epilogue writes y and the GroupNorm(1) partial of the tile for to_out.1.
//
// At the 32x32 level this replaces a 100 MB qkv round trip (to_qkv 32->384 over 65536 pixels) and two 33 MB passes by one
// read of x per kernel.  fp32 MFMA throughout (exact products), so results match the unfused kernels to summation order.
#include <cstdlib>
#include <mutex>
#include <string>

#include "common.h"
#include "stats_dev.h"

namespace fc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define FC_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int LDH = 32, LHEADS = 4, LHID = LHEADS * LDH, LC3 = 3 * LHID, PS = 33;

__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// stage rows [r0, r0+32) x channels [c0, c0+cl) of GroupNorm(x[b]) into a wave-private tile xw[32][XS]; rows >= n are zero
__device__ __forceinline__ void stage_x(const LaArgs& a, const float* Ab, const float* Bb, float* xw, int XS, int b, int r0, int c0, int cl, int lane) {
    const int q4 = cl >> 2;
    for (int idx = lane; idx < 32 * q4; idx += 64) {
        const int row = idx / q4, q = idx - row * q4, nn = r0 + row, c = c0 + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nn < a.n) {
            v = *reinterpret_cast<const float4*>(a.x + ((size_t)b * a.n + nn) * a.C + c);
            v.x = Ab[c] * v.x + Bb[c]; v.y = Ab[c + 1] * v.y + Bb[c + 1]; v.z = Ab[c + 2] * v.z + Bb[c + 2]; v.w = Ab[c + 3] * v.w + Bb[c + 3];
        }
        float* d = xw + row * XS + 4 * q;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

__global__ void __launch_bounds__(256) la_ctx_kernel(const LaArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int C = a.C, CC = C < 64 ? C : 64, XS = CC + 1;
    float* Ab = sm;
    float* Bb = Ab + C;
    float* Wl = Bb + C;                 // [C][64]: k columns | v columns of this head
    float* xt = Wl + C * 64;            // [4][32][XS]
    float* Et = xt + 4 * 32 * XS;       // [4][32][PS]
    float* Vt = Et + 4 * 32 * PS;       // [4][32][PS]
    float* sct = Vt + 4 * 32 * PS;      // [4][32]
    float* mz = sct + 128;              // [4][2][32]
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    float mean, rstd;
    combine_partials(a.xf, b, 0, &mean, &rstd);
    for (int c = tid; c < C; c += 256) {
        const float s = rstd * a.xf.gamma[c];
        Ab[c] = s;
        Bb[c] = a.xf.beta[c] - mean * s;
    }
    for (int i = tid; i < C * 64; i += 256) {
        const int c = i >> 6, j = i & 63;
        Wl[i] = a.wqkv[(size_t)c * LC3 + (j < 32 ? LHID + h * LDH + j : 2 * LHID + h * LDH + (j - 32))];
    }
    float* xw = xt + wave * 32 * XS;
    float* Ew = Et + wave * 32 * PS;
    float* Vw = Vt + wave * 32 * PS;
    float* scw = sct + wave * 32;
    const int nblk = (a.n + 31) >> 5, iters = (nblk + 3) >> 2;
    f32x16 cacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) cacc[r] = 0.f;
    float m_run = -INFINITY, z_run = 0.f;
    for (int it = 0; it < iters; ++it) {
        const int rb = it * 4 + wave, r0 = rb * 32;
        const bool active = rb < nblk;
        f32x16 ak, av;
#pragma unroll
        for (int r = 0; r < 16; ++r) { ak[r] = 0.f; av[r] = 0.f; }
        for (int c0 = 0; c0 < C; c0 += CC) {
            const int cl = C - c0 < CC ? C - c0 : CC;
            __syncthreads();
            if (active) stage_x(a, Ab, Bb, xw, XS, b, r0, c0, cl, lane);
            __syncthreads();
            if (active) {
                for (int s = 0; s < (cl >> 1); ++s) {
                    const float xa = xw[l31 * XS + 2 * s + half];
                    const float* wr = Wl + (c0 + 2 * s + half) * 64 + l31;
                    ak = FC_MFMA(xa, wr[0], ak);
                    av = FC_MFMA(xa, wr[32], av);
                }
            }
        }
        if (active) {
            float bm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) if (r0 + acc_row(r, half) < a.n) bm = fmaxf(bm, ak[r]);
            bm = fmaxf(bm, __shfl_xor(bm, 32));
            const float m_new = fmaxf(m_run, bm);
            const float sc = __expf(m_run - m_new);
            float zs = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = acc_row(r, half);
                const float e = (r0 + row < a.n) ? __expf(ak[r] - m_new) : 0.f;
                zs += e;
                Ew[row * PS + l31] = e;
                Vw[row * PS + l31] = av[r];
            }
            zs += __shfl_xor(zs, 32);
            z_run = z_run * sc + zs;
            m_run = m_new;
            if (half == 0) scw[l31] = sc;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cacc[r] *= scw[acc_row(r, half)];
#pragma unroll 4
            for (int s = 0; s < 16; ++s) cacc = FC_MFMA(Ew[(2 * s + half) * PS + l31], Vw[(2 * s + half) * PS + l31], cacc);
        }
    }
    // merge the four waves' (max, sum, context)
    __syncthreads();
    if (half == 0) { mz[(wave * 2) * 32 + l31] = m_run; mz[(wave * 2 + 1) * 32 + l31] = z_run; }
    __syncthreads();
    if (tid < 128) {
        const int w = tid >> 5, d = tid & 31;
        float M = mz[d];
        for (int k = 1; k < 4; ++k) M = fmaxf(M, mz[(k * 2) * 32 + d]);
        float Z = 0.f;
        for (int k = 0; k < 4; ++k) Z += mz[(k * 2 + 1) * 32 + d] * __expf(mz[(k * 2) * 32 + d] - M);
        sct[w * 32 + d] = __expf(mz[(w * 2) * 32 + d] - M) / Z;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = acc_row(r, half);
        Et[(wave * 32 + d) * PS + l31] = cacc[r] * sct[wave * 32 + d];
    }
    __syncthreads();
    for (int i = tid; i < LDH * LDH; i += 256) {
        const int d = i >> 5, e = i & 31;
        a.ctx[((size_t)(b * LHEADS + h) * LDH + d) * LDH + e] = (Et[d * PS + e] + Et[(32 + d) * PS + e]) + (Et[(64 + d) * PS + e] + Et[(96 + d) * PS + e]);
    }
}

template <int CT>   // CT = ceil(C / 32) output-channel tiles of to_out
__global__ void __launch_bounds__(256) la_apply_kernel(const LaArgs a, int T, float n_t) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int C = a.C, CC = C < 64 ? C : 64, XS = CC + 1, WO = CT * 32;
    const int wc_floats = CC * LHID > 32 * WO ? CC * LHID : 32 * WO;
    float* Ab = sm;
    float* Bb = Ab + C;
    float* Wc = Bb + C;                   // [CC][128] (Wq chunk), later [32][WO] (one head's rows of Wout)
    float* xt = Wc + wc_floats;           // [4][32][XS]
    float* Pt = xt + 4 * 32 * XS;         // [4][32][PS]
    float* ctxl = Pt + 4 * 32 * PS;       // [4][32][PS]
    __shared__ float red[4];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int r0 = tile * 128 + wave * 32;
    float mean, rstd;
    combine_partials(a.xf, b, 0, &mean, &rstd);
    for (int c = tid; c < C; c += 256) {
        const float s = rstd * a.xf.gamma[c];
        Ab[c] = s;
        Bb[c] = a.xf.beta[c] - mean * s;
    }
    for (int i = tid; i < LHEADS * LDH * LDH; i += 256) ctxl[(i >> 5) * PS + (i & 31)] = a.ctx[(size_t)b * LHEADS * LDH * LDH + i];
    float* xw = xt + wave * 32 * XS;
    float* Pw = Pt + wave * 32 * PS;
    f32x16 q[LHEADS];
#pragma unroll
    for (int hh = 0; hh < LHEADS; ++hh)
#pragma unroll
        for (int r = 0; r < 16; ++r) q[hh][r] = 0.f;
    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cl = C - c0 < CC ? C - c0 : CC;
        __syncthreads();
        for (int i = tid; i < cl * (LHID / 4); i += 256) {
            const int cc = i / (LHID / 4), j = (i - cc * (LHID / 4)) * 4;
            *reinterpret_cast<float4*>(Wc + cc * LHID + j) = *reinterpret_cast<const float4*>(a.wqkv + (size_t)(c0 + cc) * LC3 + j);
        }
        stage_x(a, Ab, Bb, xw, XS, b, r0, c0, cl, lane);
        __syncthreads();
        for (int s = 0; s < (cl >> 1); ++s) {
            const float xa = xw[l31 * XS + 2 * s + half];
            const float* wr = Wc + (2 * s + half) * LHID + l31;
#pragma unroll
            for (int hh = 0; hh < LHEADS; ++hh) q[hh] = FC_MFMA(xa, wr[hh * 32], q[hh]);
        }
    }
    // softmax over the 32 head channels of every (row, head): a row's channels sit in the 32 lanes of one half-wave
    const float scale = 0.17677669529663687f;
#pragma unroll
    for (int hh = 0; hh < LHEADS; ++hh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = q[hh][r];
            float m = v;
            m = fmaxf(m, __shfl_xor(m, 1)); m = fmaxf(m, __shfl_xor(m, 2)); m = fmaxf(m, __shfl_xor(m, 4));
            m = fmaxf(m, __shfl_xor(m, 8)); m = fmaxf(m, __shfl_xor(m, 16));
            const float e = __expf(v - m);
            float s = e;
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8); s += __shfl_xor(s, 16);
            q[hh][r] = e * (scale / s);
        }
    f32x16 y[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[ct][r] = 0.f;
#pragma unroll
    for (int hh = 0; hh < LHEADS; ++hh) {
        __syncthreads();
        for (int i = tid; i < 32 * WO; i += 256) {
            const int k = i / WO, c = i - k * WO;
            Wc[i] = c < C ? a.wout[(size_t)(hh * LDH + k) * C + c] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) Pw[acc_row(r, half) * PS + l31] = q[hh][r];
        __syncthreads();
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) o = FC_MFMA(Pw[l31 * PS + 2 * s + half], ctxl[(hh * LDH + 2 * s + half) * PS + l31], o);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) Pw[acc_row(r, half) * PS + l31] = o[r];
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < 16; ++s) {
            const float oa = Pw[l31 * PS + 2 * s + half];
            const float* wr = Wc + (2 * s + half) * WO + l31;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) y[ct] = FC_MFMA(oa, wr[ct * 32], y[ct]);
        }
    }
    // statistics before the stores: a barrier after them would wait for the store round trip
    float S = 0.f, Q = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 32 + l31;
        const float bias = (c < C && a.bout) ? a.bout[c] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = y[ct][r] + bias;
            y[ct][r] = v;
            if (r0 + acc_row(r, half) < a.n && c < C) { S += v; Q += v * v; }
        }
    }
    const float St = block_sum(S, red);
    const float Qt = block_sum(Q, red);
    if (tid == 0) {
        const float mt = St / n_t;
        float* d = a.stats_out + ((size_t)b * T + tile) * 2;
        d[0] = mt;
        d[1] = Qt - St * mt;
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int nn = r0 + acc_row(r, half);
            if (nn < a.n && c < C) a.y[((size_t)b * a.n + nn) * C + c] = y[ct][r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fast path, C in {8, 16, 32, 64} (every n >= 256 level of the dim 16 / 32 models).  The dependent MFMA phases of both kernels hand
// their results on IN REGISTERS: a 32x32 accumulator (lane = column, registers = rows acc_row(r, half)) is already a legal B operand
// of the next product (B[k][n]: lane = n, k chosen by half) once that product walks its reduction index in the order
// k_r = acc_row(r, half) -- and a legal A operand of a transposed product in the same way.  The reduction order is free as long as the
// other operand uses the same permutation, so no accumulator is ever stored to LDS and read back transposed.  The projections walk the
// input channels in the order c_s = s + half * C/2: a lane then needs a contiguous half row of x, which it reads straight from global
// memory (16-byte loads, normalised in registers) -- no x tile in LDS either.
//
// a lane's half row of x[b][r0 + l31]: channels [half * C/2, half * C/2 + C/2), NQ = C / 8 float4 loads; rows >= n are zero
// (NFIX != 0: n = NFIX is a constant of the instantiation and every row exists -- the plan-shape instantiations below)
template <int NQ, int NFIX = 0>
__device__ __forceinline__ void fetch_xh(const LaArgs& a, int b, int r0, int lane, float4 (&pre)[NQ]) {
    const int nn = r0 + (lane & 31), n = NFIX ? NFIX : a.n;
    const float* p = a.x + ((size_t)b * n + nn) * (NQ * 8) + (lane >> 5) * (NQ * 4);
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        if (NFIX) { pre[j] = *reinterpret_cast<const float4*>(p + 4 * j); continue; }
        pre[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nn < a.n) pre[j] = *reinterpret_cast<const float4*>(p + 4 * j);
    }
}
// GroupNorm of the half row: xn[s] = channel c_s of the lane's position (Ab / Bb: the norm's scale and shift per channel, LDS)
template <int NQ, int NFIX = 0>
__device__ __forceinline__ void norm_xh(const LaArgs& a, const float* Ab, const float* Bb, int r0, int lane, const float4 (&pre)[NQ], float (&xn)[NQ * 4]) {
    const bool in = NFIX ? true : r0 + (lane & 31) < a.n;
    const float* ap = Ab + (lane >> 5) * (NQ * 4);
    const float* bp = Bb + (lane >> 5) * (NQ * 4);
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const float4 A = *reinterpret_cast<const float4*>(ap + 4 * j), Bv = *reinterpret_cast<const float4*>(bp + 4 * j);
        float4 v = pre[j];
        if (in) { v.x = A.x * v.x + Bv.x; v.y = A.y * v.y + Bv.y; v.z = A.z * v.z + Bv.z; v.w = A.w * v.w + Bv.w; }
        xn[4 * j] = v.x; xn[4 * j + 1] = v.y; xn[4 * j + 2] = v.z; xn[4 * j + 3] = v.w;
    }
}

// NW = waves per workgroup (4 or 8).  Eight where a (sample, head) has at least eight 32-position blocks: the workgroup is the only one
// on its CU, so with four waves every SIMD held ONE wave and nothing covered its softmax arithmetic between the matrix phases; with
// eight, two waves share a SIMD's matrix pipe.  The split over positions stays inside the workgroup (the merge of the partial
// (max, sum, context) triples is one LDS pass over NW entries).
//
// Per 32-position tile: K = X Wk and V = X Wv (lane = channel, registers = positions; the lane's C weights live in registers for the
// life of the kernel), E = exp(K - m) in K's registers, then the context TRANSPOSED, ctxT[e][d] += sum_pos V[pos][e] E[pos][d], with
// A = V's and B = E's accumulator as they sit.  Transposed, the softmax channel d is the LANE of the context accumulator, so the online
// rescale by exp(m_old - m_new) is one multiply by a value the lane already holds.  Nothing in the loop touches LDS but Ab / Bb.
// NB != 0: a PLAN-SHAPE instantiation -- n = 32 NB is a constant (the dim-32 plan's n = 1024 and n = 256 levels).  The tile loop then has
// NB / NW trips, known when the kernel is compiled: every x tile of the wave is requested before the first wait (no global load inside a
// loop with a run-time trip count, section 7 of DESIGN.md), and no accumulator row is masked (n is a multiple of 32).  Same values, same
// order of every sum as the run-time form (NB = 0), which serves every other shape.
template <int NQ, int NW, int NB = 0>
__global__ void __launch_bounds__(64 * NW) la_ctx_fast_kernel(const LaArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int C = NQ * 8, H2 = C / 2, NT = 64 * NW;
    constexpr bool FIX = NB != 0;
    constexpr int NFIX = NB * 32, ITER = FIX ? NB / NW : 1;
    static_assert(!FIX || (NB % NW == 0 && NB >= NW), "plan-shape instantiation: whole rounds of the workgroup's waves");
    float* Ab = sm;
    float* Bb = Ab + C;
    float* Et = Bb + C;                 // [NW][32][PS]
    float* sct = Et + NW * 32 * PS;     // [NW][32]
    float* mz = sct + NW * 32;          // [NW][2][32]
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int nblk = FIX ? NB : (a.n + 31) >> 5;
    // every cold operand is requested before anything is waited for: first x tile (plan shape: every x tile), statistics, norm parameters, weights
    float4 pre[ITER][NQ];
    if constexpr (FIX) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) fetch_xh<NQ, NFIX>(a, b, (wave + it * NW) * 32, lane, pre[it]);
    } else {
        if (wave < nblk) fetch_xh<NQ>(a, b, wave * 32, lane, pre[0]);
    }
    PartPre pp;
    partials_request(a.xf, b, 0, pp);
    const float pg = tid < C ? a.xf.gamma[tid] : 0.f, pbt = tid < C ? a.xf.beta[tid] : 0.f;   // C <= 64 < 256 threads
    float wk[H2], wv[H2];               // B operands: lane (column l31, half) supplies channel c_s of its k / v column
#pragma unroll
    for (int s = 0; s < H2; ++s) {
        const float* wr = a.wqkv + (size_t)(s + half * H2) * LC3 + h * LDH + l31;
        wk[s] = wr[LHID];
        wv[s] = wr[2 * LHID];
    }
    float mean, rstd;
    partials_finish(a.xf, b, 0, pp, &mean, &rstd);
    if (tid < C) {
        const float s = rstd * pg;
        Ab[tid] = s;
        Bb[tid] = pbt - mean * s;
    }
    __syncthreads();
    f32x16 cacc;                        // ctxT: lane = d, registers = e
#pragma unroll
    for (int r = 0; r < 16; ++r) cacc[r] = 0.f;
    float m_run = -INFINITY, z_run = 0.f;
    // one 32-position tile: k, v, online softmax over the positions, context
    auto tile = [&](const int r0, const float (&xn)[H2]) {
        f32x16 ak, av;
#pragma unroll
        for (int r = 0; r < 16; ++r) { ak[r] = 0.f; av[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < H2; ++s) {
            ak = FC_MFMA(xn[s], wk[s], ak);
            av = FC_MFMA(xn[s], wv[s], av);
        }
        float bm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) if (FIX || r0 + acc_row(r, half) < a.n) bm = fmaxf(bm, ak[r]);
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float m_new = fmaxf(m_run, bm);
        const float sc = __expf(m_run - m_new);
        float zs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = (FIX || r0 + acc_row(r, half) < a.n) ? __expf(ak[r] - m_new) : 0.f;
            zs += e;
            ak[r] = e;
        }
        zs += __shfl_xor(zs, 32);
        z_run = z_run * sc + zs;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) cacc[r] *= sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) cacc = FC_MFMA(av[r], ak[r], cacc);
    };
    if constexpr (FIX) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int r0 = (wave + it * NW) * 32;
            float xn[H2];
            norm_xh<NQ, NFIX>(a, Ab, Bb, r0, lane, pre[it], xn);
            tile(r0, xn);
        }
    } else {
        for (int rb = wave; rb < nblk; rb += NW) {
            const int r0 = rb * 32;
            float xn[H2];
            norm_xh<NQ>(a, Ab, Bb, r0, lane, pre[0], xn);
            if (rb + NW < nblk) fetch_xh<NQ>(a, b, r0 + 32 * NW, lane, pre[0]);
            tile(r0, xn);
        }
    }
    if (half == 0) { mz[(wave * 2) * 32 + l31] = m_run; mz[(wave * 2 + 1) * 32 + l31] = z_run; }
    __syncthreads();
    if (tid < 32 * NW) {
        const int w = tid >> 5, d = tid & 31;
        float M = mz[d];
        for (int k = 1; k < NW; ++k) M = fmaxf(M, mz[(k * 2) * 32 + d]);
        float Z = 0.f;
        for (int k = 0; k < NW; ++k) Z += mz[(k * 2 + 1) * 32 + d] * __expf(mz[(k * 2) * 32 + d] - M);
        sct[w * 32 + d] = __expf(mz[(w * 2) * 32 + d] - M) / Z;
    }
    __syncthreads();
    const float fw = sct[wave * 32 + l31];
#pragma unroll
    for (int r = 0; r < 16; ++r) Et[(wave * 32 + l31) * PS + acc_row(r, half)] = cacc[r] * fw;
    __syncthreads();
    for (int i = tid; i < LDH * LDH; i += NT) {
        const int d = i >> 5, e = i & 31;
        float v = (Et[d * PS + e] + Et[(32 + d) * PS + e]) + (Et[(64 + d) * PS + e] + Et[(96 + d) * PS + e]);
        if (NW == 8) v += (Et[(128 + d) * PS + e] + Et[(160 + d) * PS + e]) + (Et[(192 + d) * PS + e] + Et[(224 + d) * PS + e]);
        a.ctx[((size_t)(b * LHEADS + h) * LDH + d) * LDH + e] = v;
    }
}

// One 128-position tile per workgroup, 32 positions per wave, everything computed TRANSPOSED so that lane = position throughout:
//   qT[d][pos]   = sum_c WqT[d][c] xnT[c][pos]        A = Wq, B = the lane's normalised half row          -> lane = pos, registers = d
//   softmax over d: sixteen registers and one exchange with lane ^ 32, in place
//   outT[e][pos] = sum_d ctxT[e][d] P[d][pos]         A = context, B = the softmax result as it sits        -> registers = e
//   yT[c][pos]  += sum_e WoT[c][e] outT[e][pos]       A = Wout, B = the out accumulator as it sits          -> registers = c
// one head at a time.  The A operands (the same for every wave) are staged once in LDS in the order each lane consumes them -- the
// reduction index permuted to k_r = acc_row(r, half) -- with a row stride of (steps + 4) floats, so that four k-steps are one
// conflict-free 16-byte read.  yT leaves a lane with 16 channels of its position in four runs of four: bias, statistics, the fused
// close and the stores work on 16-byte channel quads.
constexpr int AS = 20;                  // row stride of a 16-step A operand image
__device__ __forceinline__ int acc_reg(int row) { return (row & 3) + 4 * (row >> 3); }   // acc_row(acc_reg(row), (row >> 2) & 1) == row
// TT != 0: a PLAN-SHAPE instantiation -- the sample has exactly TT tiles (n = 128 TT), a constant.  No row is masked, the epoch is a shift
// of the arrival count, a thread polls at most one granule under a constant bound, the close is a straight line of TT terms in the run-time
// form's order, and the two block sums share one pair of barriers (each quantity's additions in block_sum's order).
template <int NQ, int CT, int TT = 0>
__global__ void __launch_bounds__(256) la_apply_fast_kernel(const LaArgs a, int T_rt, float n_t) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int C = NQ * 8, H2 = C / 2, SQ = H2 + 4, WO = CT * 32;
    constexpr bool FIX = TT != 0;
    constexpr int NFIX = TT * 128;
    static_assert(TT <= kPartPre, "one granule pair per tile, polled by 2 TT threads");
    const int T = FIX ? TT : T_rt, n = FIX ? NFIX : a.n;
    float* Ab = sm;
    float* Bb = Ab + C;
    float* WqL = Bb + C;                          // [4 heads][half][32 d][SQ]: Wq[c_s][h * 32 + d] at s
    float* ctxL = WqL + LHEADS * 64 * SQ;         // [4][half][32 e][AS]: ctx[h][acc_row(r, half)][e] at r
    float* WoL = ctxL + LHEADS * 64 * AS;         // [4][CT][half][32 c][AS]: Wout[h * 32 + acc_row(r, half)][ct * 32 + c] at r
    __shared__ float red[4], red2[4];
    __shared__ unsigned epoch_s;
    __shared__ float gv[2 * kPartPre];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int r0 = tile * 128 + wave * 32, nn = r0 + l31;
    const bool in = FIX ? true : nn < a.n;
    // the fused close (a.gran; T <= kPartPre): this launch's epoch from the sample's arrival counter
    unsigned arrival = 0;
    if (a.gran && tid == 0) arrival = __hip_atomic_fetch_add(a.sync + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every cold operand is requested before anything is waited for: x, statistics, norm parameters, weights, context
    float4 pre[NQ];
    fetch_xh<NQ, NFIX>(a, b, r0, lane, pre);
    PartPre pp;
    partials_request(a.xf, b, 0, pp);
    const float pg = tid < C ? a.xf.gamma[tid] : 0.f, pbt = tid < C ? a.xf.beta[tid] : 0.f;   // C <= 64 < 256 threads
    // Wq, Wout and the context into explicit registers first, LDS after: as load -> store loops they are dependent round trips
    constexpr int NWO = WO / 2;
    float4 wq[NQ], cx[4];
    float wo[NWO];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int i = tid + 256 * k, cc = (i >> 7) * 4 + (i & 3), j = ((i >> 2) & 31) * 4;   // four channels x 16 column quads per wave: LDS store banks
        wq[k] = *reinterpret_cast<const float4*>(a.wqkv + (size_t)cc * LC3 + j);
    }
#pragma unroll
    for (int k = 0; k < NWO; ++k) {
        const int i = tid + 256 * k, kk = i / WO, c = i - kk * WO;
        wo[k] = c < C ? a.wout[(size_t)kk * C + c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = *reinterpret_cast<const float4*>(a.ctx + (size_t)b * LHEADS * LDH * LDH + 4 * (tid + 256 * k));
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int i = tid + 256 * k, cc = (i >> 7) * 4 + (i & 3), j = ((i >> 2) & 31) * 4;
        const int hf = cc / H2, s = cc - hf * H2;
        float* d = WqL + (((j >> 5) * 2 + hf) * 32 + (j & 31)) * SQ + s;
        d[0] = wq[k].x; d[SQ] = wq[k].y; d[2 * SQ] = wq[k].z; d[3 * SQ] = wq[k].w;
    }
#pragma unroll
    for (int k = 0; k < NWO; ++k) {
        const int i = tid + 256 * k, kk = i / WO, c = i - kk * WO, e = kk & 31;
        WoL[((((kk >> 5) * CT + (c >> 5)) * 2 + ((e >> 2) & 1)) * 32 + (c & 31)) * AS + acc_reg(e)] = wo[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = 4 * (tid + 256 * k), d0 = (i >> 5) & 31;
        float* d = ctxL + (((i >> 10) * 2 + ((d0 >> 2) & 1)) * 32 + (i & 31)) * AS + acc_reg(d0);
        d[0] = cx[k].x; d[AS] = cx[k].y; d[2 * AS] = cx[k].z; d[3 * AS] = cx[k].w;
    }
    {
        float mean, rstd;
        partials_finish(a.xf, b, 0, pp, &mean, &rstd);
        if (tid < C) {
            const float s = rstd * pg;
            Ab[tid] = s;
            Bb[tid] = pbt - mean * s;
        }
        if (a.gran && tid == 0) epoch_s = arrival / (unsigned)T + 1u;
    }
    // the close's operands depend on nothing computed here: to_out.0's bias and the residual are requested now
    float4 pbias[CT][4], rs[CT][4];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = ct * 32 + 8 * g + 4 * half;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            pbias[ct][g] = z; rs[ct][g] = z;
            if (c < C && a.bout) pbias[ct][g] = *reinterpret_cast<const float4*>(a.bout + c);
            if (a.gran && c < C && in) rs[ct][g] = *reinterpret_cast<const float4*>(a.x + ((size_t)b * n + nn) * C + c);
        }
    __syncthreads();
    float xn[H2];
    norm_xh<NQ, NFIX>(a, Ab, Bb, r0, lane, pre, xn);
    const float scale = 0.17677669529663687f;
    f32x16 y[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[ct][r] = 0.f;
#pragma unroll
    for (int hh = 0; hh < LHEADS; ++hh) {
        f32x16 q;
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] = 0.f;
        const float* wa = WqL + ((hh * 2 + half) * 32 + l31) * SQ;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const float4 w = *reinterpret_cast<const float4*>(wa + 4 * j);
            q = FC_MFMA(w.x, xn[4 * j], q);
            q = FC_MFMA(w.y, xn[4 * j + 1], q);
            q = FC_MFMA(w.z, xn[4 * j + 2], q);
            q = FC_MFMA(w.w, xn[4 * j + 3], q);
        }
        // softmax over the head's 32 channels: this lane holds 16 of them, lane ^ 32 the other 16 of the same position
        float m = q[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) m = fmaxf(m, q[r]);
        m = fmaxf(m, __shfl_xor(m, 32));
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { q[r] = __expf(q[r] - m); sum += q[r]; }
        sum += __shfl_xor(sum, 32);
        const float f = scale / sum;
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] *= f;
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
        const float* ca = ctxL + ((hh * 2 + half) * 32 + l31) * AS;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 w = *reinterpret_cast<const float4*>(ca + 4 * j);
            o = FC_MFMA(w.x, q[4 * j], o);
            o = FC_MFMA(w.y, q[4 * j + 1], o);
            o = FC_MFMA(w.z, q[4 * j + 2], o);
            o = FC_MFMA(w.w, q[4 * j + 3], o);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const float* oa = WoL + (((hh * CT + ct) * 2 + half) * 32 + l31) * AS;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 w = *reinterpret_cast<const float4*>(oa + 4 * j);
                y[ct] = FC_MFMA(w.x, o[4 * j], y[ct]);
                y[ct] = FC_MFMA(w.y, o[4 * j + 1], y[ct]);
                y[ct] = FC_MFMA(w.z, o[4 * j + 2], y[ct]);
                y[ct] = FC_MFMA(w.w, o[4 * j + 3], y[ct]);
            }
        }
    }
    // y[ct][4 g + i] is channel ct * 32 + 8 g + 4 half + i of position nn.  Statistics before the stores: a barrier after them would
    // wait for the store round trip
    float S = 0.f, Q = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bi = pbias[ct][g];
            const float v0 = y[ct][4 * g] + bi.x, v1 = y[ct][4 * g + 1] + bi.y, v2 = y[ct][4 * g + 2] + bi.z, v3 = y[ct][4 * g + 3] + bi.w;
            y[ct][4 * g] = v0; y[ct][4 * g + 1] = v1; y[ct][4 * g + 2] = v2; y[ct][4 * g + 3] = v3;
            if (in && ct * 32 + 8 * g + 4 * half < C) {
                S += v0; Q += v0 * v0; S += v1; Q += v1 * v1; S += v2; Q += v2 * v2; S += v3; Q += v3 * v3;
            }
        }
    float St, Qt;
    if constexpr (FIX) {                // both sums over one pair of barriers; each one's additions in block_sum's order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { S += __shfl_xor(S, o); Q += __shfl_xor(Q, o); }
        __syncthreads();
        if (lane == 0) { red[wave] = S; red2[wave] = Q; }
        __syncthreads();
        St = red[0] + red[1] + red[2] + red[3];
        Qt = red2[0] + red2[1] + red2[2] + red2[3];
    } else {
        St = block_sum(S, red);
        Qt = block_sum(Q, red);
    }
    if (a.gran) {
        // ---- the module closed here: out = GroupNorm(1)(y) * g2 + b2 + x, the statistics completed by the sample's other tiles ----
        // The partials travel as ONE 8-byte write-through store each, {epoch, bits}: the data is its own flag (the convolution tails'
        // hand-off, conv_dev.h); sc1 accesses that bypass the per-XCD L2, no fence.  finalize_kernel's arithmetic (stats_dev.h
        // partials_finish) in the same order, so the exclusive and the shared plan agree to the last bit.
        const unsigned epoch = epoch_s;
        float4 g2[CT][4], b2[CT][4];        // requested before the wait
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = ct * 32 + 8 * g + 4 * half;
                g2[ct][g] = make_float4(0.f, 0.f, 0.f, 0.f); b2[ct][g] = g2[ct][g];
                if (c < C) { g2[ct][g] = *reinterpret_cast<const float4*>(a.g2 + c); b2[ct][g] = *reinterpret_cast<const float4*>(a.b2 + c); }
            }
        if (tid == 0) {
            const float mt = St / n_t;
            unsigned long long* gp = a.gran + ((size_t)b * T + tile) * 2;
            const unsigned long long tag = (unsigned long long)epoch << 32;
            __hip_atomic_store(gp, tag | __float_as_uint(mt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(gp + 1, tag | __float_as_uint(Qt - St * mt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid < 2 * T) {          // one granule per thread, polled until it carries this launch's epoch.  Bounded: a residency mistake
                                    // must not hang the device -- the statistic becomes NaN and the handle's error word is set
            const unsigned long long* gp = a.gran + (size_t)b * T * 2 + tid;
            unsigned long long v = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int spins = 0;
            while ((unsigned)(v >> 32) != epoch) {
                if (++spins > (1 << 20)) { if (a.err) *a.err = 1; v = 0x7fc00000ull; break; }
                __builtin_amdgcn_s_sleep(2);
                v = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            gv[tid] = __uint_as_float((unsigned)v);
        }
        __syncthreads();
        float sm2 = 0.f;
        for (int t = 0; t < T; ++t) sm2 += gv[2 * t];        // (plan shape: T is a constant, a straight line)
        const float mean = sm2 / (float)T;
        float m2 = 0.f, dv = 0.f;
        for (int t = 0; t < T; ++t) {
            const float d = gv[2 * t] - mean;
            m2 += gv[2 * t + 1];
            dv += d * d;
        }
        const float rstd = 1.0f / sqrtf((m2 + n_t * dv) / (n_t * (float)T) + a.eps2);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = ct * 32 + 8 * g + 4 * half;
                const float4 gg = g2[ct][g], bb = b2[ct][g], rr = rs[ct][g];
                float4 ov;
                { const float A = rstd * gg.x, Bc = bb.x - mean * A; ov.x = (A * y[ct][4 * g] + Bc) + rr.x; }
                { const float A = rstd * gg.y, Bc = bb.y - mean * A; ov.y = (A * y[ct][4 * g + 1] + Bc) + rr.y; }
                { const float A = rstd * gg.z, Bc = bb.z - mean * A; ov.z = (A * y[ct][4 * g + 2] + Bc) + rr.z; }
                { const float A = rstd * gg.w, Bc = bb.w - mean * A; ov.w = (A * y[ct][4 * g + 3] + Bc) + rr.w; }
                if (in && c < C) *reinterpret_cast<float4*>(a.out + ((size_t)b * n + nn) * C + c) = ov;
            }
        return;
    }
    if (tid == 0) {
        const float mt = St / n_t;
        float* d = a.stats_out + ((size_t)b * T + tile) * 2;
        d[0] = mt;
        d[1] = Qt - St * mt;
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = ct * 32 + 8 * g + 4 * half;
            if (in && c < C) *reinterpret_cast<float4*>(a.y + ((size_t)b * n + nn) * C + c) = make_float4(y[ct][4 * g], y[ct][4 * g + 1], y[ct][4 * g + 2], y[ct][4 * g + 3]);
        }
}

static size_t la_ctx_fast_lds(int C, int NW) { return (size_t)(2 * C + NW * 32 * PS + 32 * NW + 64 * NW) * sizeof(float); }
static int la_ctx_waves(int n) { return n >= 256 ? 8 : 4; }      // eight waves once every one of them has a 32-position block of its own
static size_t la_apply_fast_lds(int C, int CT) { return (size_t)(2 * C + LHEADS * 64 * (C / 2 + 4) + LHEADS * 64 * AS + LHEADS * CT * 64 * AS) * sizeof(float); }
// The plan-shape instantiations (the dim-32 inference plan at 4x32x32): (C, n) -> n / 32, or 0: the run-time form.  Exact match only.
static int la_plan_nb(int C, int n) {
    if (C == 32 && n == 1024) return 32;     // downs.0.2, ups.3.2
    if (C == 32 && n == 256) return 8;       // downs.1.2
    if (C == 64 && n == 256) return 8;       // ups.2.2
    return 0;
}
// Diagnostics (fc_debug_conv_routes switches the record on and off, fc_debug_linattn_routes_read copies it): what launch_fast really
// launched, one line "C n NB TT" per module -- NB / TT are the template constants of the context / apply kernel it took (0 0: the pair
// that reads the shape at run time).
static std::mutex g_la_route_mu;
static bool g_la_route_on = false;
static std::string g_la_route_log;
void linattn_route_log_set(bool on) { std::lock_guard<std::mutex> lk(g_la_route_mu); g_la_route_on = on; if (on) g_la_route_log.clear(); }
std::string linattn_route_log_get() { std::lock_guard<std::mutex> lk(g_la_route_mu); return g_la_route_log; }
struct LaCtxSel { void (*fn)(const LaArgs); int NB; };
struct LaApplySel { void (*fn)(const LaArgs, int, float); int TT; };
// the instantiation a launch of (C = 8 NQ, n) runs: the exclusive plan, the plan on a shared device and the residency query all ask here
template <int NQ>
static LaCtxSel la_ctx_fast_for(int n) {
    if constexpr (NQ == 4) {
        if (la_plan_nb(NQ * 8, n) == 32) return {la_ctx_fast_kernel<NQ, 8, 32>, 32};
        if (la_plan_nb(NQ * 8, n) == 8) return {la_ctx_fast_kernel<NQ, 8, 8>, 8};
    }
    if constexpr (NQ == 8) {
        if (la_plan_nb(NQ * 8, n) == 8) return {la_ctx_fast_kernel<NQ, 8, 8>, 8};
    }
    if (la_ctx_waves(n) == 8) return {la_ctx_fast_kernel<NQ, 8>, 0};
    return {la_ctx_fast_kernel<NQ, 4>, 0};
}
template <int NQ>
static LaApplySel la_apply_fast_for(int n) {
    if constexpr (NQ == 4) {
        if (la_plan_nb(NQ * 8, n) == 32) return {la_apply_fast_kernel<NQ, 1, 8>, 8};
        if (la_plan_nb(NQ * 8, n) == 8) return {la_apply_fast_kernel<NQ, 1, 2>, 2};
    }
    if constexpr (NQ == 8) {
        if (la_plan_nb(NQ * 8, n) == 8) return {la_apply_fast_kernel<NQ, 2, 2>, 2};
    }
    if constexpr (NQ * 8 <= 32) return {la_apply_fast_kernel<NQ, 1>, 0};
    else return {la_apply_fast_kernel<NQ, 2>, 0};
}
template <int NQ>
static int launch_fast(const LaArgs& a, hipStream_t s) {
    const int NW = la_ctx_waves(a.n);
    const LaCtxSel cs = la_ctx_fast_for<NQ>(a.n);
    const LaApplySel as = la_apply_fast_for<NQ>(a.n);
    if (g_la_route_on) {
        std::lock_guard<std::mutex> lk(g_la_route_mu);
        g_la_route_log += std::to_string(a.C) + " " + std::to_string(a.n) + " " + std::to_string(cs.NB) + " " + std::to_string(as.TT) + "\n";
    }
    hipLaunchKernelGGL(cs.fn, dim3(LHEADS, a.B), dim3(64 * NW), la_ctx_fast_lds(a.C, NW), s, a);
    FC_HIP(hipGetLastError());
    const int T = linattn_fused_tiles(a.n);
    const float n_t = linattn_fused_nt(a.n, a.C);
    // One 128-position tile per workgroup: the A operand images of a workgroup are 61 KB of LDS at C = 32, so two workgroups share a CU
    // and two waves a SIMD -- one wave's softmax arithmetic runs under the other's matrix phases.
    const dim3 grid(cdiv(a.n, 128), a.B);
    hipLaunchKernelGGL(as.fn, grid, dim3(256), la_apply_fast_lds(a.C, a.C <= 32 ? 1 : 2), s, a, T, n_t);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
template <int NQ>
static int init_fast() {
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_ctx_fast_kernel<NQ, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_ctx_fast_kernel<NQ, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_apply_fast_kernel<NQ, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_apply_fast_kernel<NQ, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    for (int n : {256, 1024}) {          // the plan-shape instantiations (the run-time ones again where there is none)
        FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_ctx_fast_for<NQ>(n).fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_apply_fast_for<NQ>(n).fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    }
    return FC_OK;
}

static size_t la_ctx_lds(int C) {
    const int CC = C < 64 ? C : 64;
    return (size_t)(2 * C + C * 64 + 4 * 32 * (CC + 1) + 2 * 4 * 32 * PS + 128 + 256) * sizeof(float);
}
static size_t la_apply_lds(int C, int CT) {
    const int CC = C < 64 ? C : 64, WO = CT * 32;
    const int wc = CC * LHID > 32 * WO ? CC * LHID : 32 * WO;
    return (size_t)(2 * C + wc + 4 * 32 * (CC + 1) + 2 * 4 * 32 * PS) * sizeof(float);
}

int linattn_fused_tiles(int n) { return n >= 128 ? n / 128 : 1; }
float linattn_fused_nt(int n, int C) { return (float)((n >= 128 ? 128 : n) * C); }

int linattn_fused_init() {
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_ctx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_apply_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_apply_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_apply_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(la_apply_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    FC_TRY(init_fast<1>()); FC_TRY(init_fast<2>()); FC_TRY(init_fast<4>()); FC_TRY(init_fast<8>());
    return FC_OK;
}

bool linattn_fused_supported(int n, int C, int heads) {
    if (heads != LHEADS || (C & 3) || C > 256 || n < 1) return false;
    if (n >= 128 && (n & 127)) return false;
    return la_ctx_lds(C) <= 160 * 1024;
}

// May the apply launch close the module itself (LaArgs::gran)?  Its workgroups wait for the other tiles of their sample, so every
// workgroup of the grid must be resident at once: occupancy of the kernel at this C times the CU count >= tiles * B.  Fast path only.
template <int NQ>
static int apply_blocks_per_cu(int C, int n) {      // of the instantiation launch_fast runs at this shape
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, la_apply_fast_for<NQ>(n).fn, 256, la_apply_fast_lds(C, C <= 32 ? 1 : 2));
    return e == hipSuccess ? nb : 0;
}
bool linattn_fused_meeting_ok(int B, int n, int C) {
    if (n < 256 || (n & 127) || !(C == 8 || C == 16 || C == 32 || C == 64)) return false;
    const int T = linattn_fused_tiles(n);
    if (T != n / 128 || T > kPartPre) return false;
    if (linattn_fused_init() != FC_OK) return false;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
    const int per = C == 8 ? apply_blocks_per_cu<1>(C, n) : C == 16 ? apply_blocks_per_cu<2>(C, n) : C == 32 ? apply_blocks_per_cu<4>(C, n) : apply_blocks_per_cu<8>(C, n);
    return (long long)per * cus >= (long long)T * B;
}

int linattn_fused_launch(const LaArgs& a, hipStream_t s) {
    if (!linattn_fused_supported(a.n, a.C, a.heads)) return fail(FC_E_SHAPE, "linattn_fused: unsupported shape");
    if (a.xf.mode != 1 || a.xf.G != 1 || !a.xf.stats) return fail(FC_E_ARG, "linattn_fused: needs GroupNorm(1) statistics of x");
    if (a.gran && (!a.sync || !a.out || !a.g2 || !a.b2 || !(a.C == 8 || a.C == 16 || a.C == 32 || a.C == 64)))
        return fail(FC_E_ARG, "linattn_fused: the fused close needs the fast path, the arrival counters, to_out.1's parameters and the output");
    if (a.C <= 64 && (a.C & 7) == 0 && (a.C == 8 || a.C == 16 || a.C == 32 || a.C == 64)) {
        switch (a.C) {
            case 8: return launch_fast<1>(a, s);
            case 16: return launch_fast<2>(a, s);
            case 32: return launch_fast<4>(a, s);
            default: return launch_fast<8>(a, s);
        }
    }
    hipLaunchKernelGGL(la_ctx_kernel, dim3(LHEADS, a.B), dim3(256), la_ctx_lds(a.C), s, a);
    FC_HIP(hipGetLastError());
    const int T = linattn_fused_tiles(a.n);
    const float n_t = linattn_fused_nt(a.n, a.C);
    const int CT = a.C <= 32 ? 1 : a.C <= 64 ? 2 : a.C <= 128 ? 4 : 8;
    const dim3 grid(cdiv(a.n, 128), a.B);
    const size_t lds = la_apply_lds(a.C, CT);
    switch (CT) {
        case 1: hipLaunchKernelGGL(la_apply_kernel<1>, grid, dim3(256), lds, s, a, T, n_t); break;
        case 2: hipLaunchKernelGGL(la_apply_kernel<2>, grid, dim3(256), lds, s, a, T, n_t); break;
        case 4: hipLaunchKernelGGL(la_apply_kernel<4>, grid, dim3(256), lds, s, a, T, n_t); break;
        default: hipLaunchKernelGGL(la_apply_kernel<8>, grid, dim3(256), lds, s, a, T, n_t); break;
    }
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // namespace fc
