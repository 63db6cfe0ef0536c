// Set distances between sample sets (no upstream counterpart; DESIGN.md section 4 "Set distances").
//
//   Frechet:  FD = |mx - my|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2),   tr sqrt(S1 S2) = ||A B^T||_*  (nuclear norm),
//             A = (X - mx) / sqrt(N1 - 1), B = (Y - my) / sqrt(N2 - 1): no D x D matrix exists, D is the inner extent of one fp64 Gram.
//   KID:      the unbiased MMD^2 with k(x, y) = (x.y / D + 1)^3 from three Gram launches whose epilogue reduces instead of storing.
//   Moments:  for N >> D a set is (n, mean, M = sum (x - mean)(x - mean)^T), fed batch by batch (scatter_kernel: the batch's centred
//             scatter on the same MFMA, joined by Chan's pairwise rule), S = M / (n - 1) = F^T F with F from the Jacobi iteration run on the
//             rows of S, and tr sqrt(S1 S2) = ||F1 F2^T||_*: one fp64 Gram of two factors (gram_kernel on fp64 rows) and a third solve.
//
// Kernels: gram_kernel (fp32 rows, centred in fp64 on load, v_mfma_f64_16x16x4_f64, 32 x 32 tile per workgroup of four waves, LDS tiled
// over the features, every edge predicated), col_moments_kernel (fp64 mean per feature and sum |x - mean|^2), jacobi_pair_kernel (one
// launch per round of the round-robin schedule, one workgroup per pair of vectors, never waits for another workgroup), svals_kernel
// (norms -> sorted singular values and their sum).  Every sum has a fixed order: the same bits run to run.  The only atomics are the
// integer rotation counters.
#include <math.h>

#include "common.h"

namespace fc {

constexpr int GR_T = 32, GR_BK = 32, GR_LD = GR_BK + 1, GR_THREADS = 256;
constexpr int JC_THREADS = 256, JC_MAX_N = FC_FRECHET_MAX_SMALL;
constexpr int CM_F = 32, CM_R = 8;                    // col_moments: features x row lanes of a workgroup
typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over the 256 threads of a workgroup in a fixed order (xor tree inside a wave, then waves 0..3); sh: 4 doubles, reusable after return
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ------------------------------------------------------------------------------------------------ Gram
template <typename T>
struct GramArgsT {
    const T *a, *b;              // [n1][dim], [n2][dim]: fp32 sample rows, or the fp64 rows of two covariance factors
    const double *ma, *mb;       // [dim] or null
    int n1, n2;
    long long dim;
    double scale;
    double* c;                   // [n1][n2] (store mode)
    double* part;                // one fp64 per workgroup or null: sum of the stored values squared (store), sum of k (reduce)
    int skip_diag;
};
using GramArgs = GramArgsT<float>;

// C = scale (a - ma)(b - mb)^T.  The f64 MFMA's lane maps: lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one
// f64 each, and holds C[row = (l >> 4) + 4 reg][col = l & 15] in reg 0..3 (not the fp32 shapes' row map).
template <bool REDUCE, typename T>
__global__ void __launch_bounds__(GR_THREADS) gram_kernel(const GramArgsT<T> g) {
    __shared__ double As[GR_T * GR_LD], Bs[GR_T * GR_LD];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i0 = blockIdx.y * GR_T, j0 = blockIdx.x * GR_T;
    const int lr = tid >> 5, lc = tid & 31;                   // this thread stages rows lr + 8 q, feature lc of a chunk
    double ra[4], rb[4];
    auto load = [&](long long f0) {
        const long long f = f0 + lc;
        const bool fok = f < g.dim;
        const double ca = (fok && g.ma) ? g.ma[f] : 0.0, cb = (fok && g.mb) ? g.mb[f] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ia = i0 + lr + 8 * q, ib = j0 + lr + 8 * q;
            ra[q] = (fok && ia < g.n1) ? (double)g.a[(size_t)ia * g.dim + f] - ca : 0.0;
            rb[q] = (fok && ib < g.n2) ? (double)g.b[(size_t)ib * g.dim + f] - cb : 0.0;
        }
    };
    const int wi = (w >> 1) * 16, wj = (w & 1) * 16;
    const int ar = (wi + (lane & 15)) * GR_LD + (lane >> 4), br = (wj + (lane & 15)) * GR_LD + (lane >> 4);
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    load(0);
    for (long long f0 = 0; f0 < g.dim; f0 += GR_BK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            As[(lr + 8 * q) * GR_LD + lc] = ra[q];
            Bs[(lr + 8 * q) * GR_LD + lc] = rb[q];
        }
        __syncthreads();
        if (f0 + GR_BK < g.dim) load(f0 + GR_BK);
#pragma unroll
        for (int kk = 0; kk < GR_BK / 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[ar + 4 * kk], Bs[br + 4 * kk], acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = j0 + wj + (lane & 15);
    double s = 0.0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = i0 + wi + (lane >> 4) + 4 * reg;
        if (row >= g.n1 || col >= g.n2) continue;
        if (REDUCE) {
            if (g.skip_diag && row == col) continue;
            const double t = acc[reg] / (double)g.dim + 1.0;
            s += t * t * t;
        } else {
            const double v = g.scale * acc[reg];
            g.c[(size_t)row * g.n2 + col] = v;
            s += v * v;
        }
    }
    if (g.part) {
        s = block_sum(s, red);
        if (tid == 0) g.part[blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// out[0] = sum of part[0..n) in a fixed order: thread t takes t, t + 256, ..., then the workgroup's tree
__global__ void __launch_bounds__(256) sum_partials_kernel(const double* part, long long n, double* out) {
    __shared__ double red[4];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// ------------------------------------------------------------------------------------------------ moments
// mean[f] = sum_i x[i][f] / n (row lane ry adds rows ry, ry + 8, ... in order, the eight lanes are added 0..7), and per workgroup
// part[block] = sum over its 32 features and all rows of (x - mean)^2
__global__ void __launch_bounds__(CM_F * CM_R) col_moments_kernel(const float* x, int n, long long dim, double* mean, double* part) {
    __shared__ double sh[CM_R][CM_F];
    __shared__ double red[4];
    const int fx = threadIdx.x & (CM_F - 1), ry = threadIdx.x / CM_F;
    const long long f = (long long)blockIdx.x * CM_F + fx;
    double s = 0.0;
    if (f < dim)
        for (int row = ry; row < n; row += CM_R) s += (double)x[(size_t)row * dim + f];
    sh[ry][fx] = s;
    __syncthreads();
    double m = sh[0][fx];
#pragma unroll
    for (int q = 1; q < CM_R; ++q) m += sh[q][fx];
    m /= (double)n;
    if (ry == 0 && f < dim) mean[f] = m;
    double q2 = 0.0;
    if (f < dim)
        for (int row = ry; row < n; row += CM_R) {
            const double d = (double)x[(size_t)row * dim + f] - m;
            q2 += d * d;
        }
    q2 = block_sum(q2, red);
    if (threadIdx.x == 0) part[blockIdx.x] = q2;
}

__global__ void __launch_bounds__(256) mean_diff2_kernel(const double* mx, const double* my, long long dim, double* out) {
    __shared__ double red[4];
    double s = 0.0;
    for (long long f = threadIdx.x; f < dim; f += 256) {
        const double d = mx[f] - my[f];
        s += d * d;
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// ------------------------------------------------------------------------------------------------ one-sided Jacobi
struct JacobiArgs {
    double* z;                   // [n][r], vector i contiguous
    int n, m, r, round;          // m = n rounded up to even: index n (odd n) is the zero padding vector, whose pairs have nothing to do
    const double* fro2;          // ||Z||_F^2 of the input
    int* counter;                // this sweep's {rotations, pairs with a non-finite product}
};

// Round `round` (0 .. m - 2) of the circle schedule: pair 0 is (m - 1, round), pair p is (round + p, round - p) mod (m - 1).
// LDS: both vectors stay in the workgroup's LDS between the products and the rotation (r <= FC_JACOBI_LDS_R); else the rotation
// reads them from memory a second time.
template <bool LDS>
__global__ void __launch_bounds__(JC_THREADS) jacobi_pair_kernel(const JacobiArgs j) {
    extern __shared__ double vec[];                                 // LDS: [2][r]
    __shared__ double red[12];
    const int p = blockIdx.x, m1 = j.m - 1, tid = threadIdx.x;
    int ia = p == 0 ? m1 : (j.round + p) % m1, ib = p == 0 ? j.round : (j.round - p + m1) % m1;
    if (ia >= j.n || ib >= j.n) return;                             // the padding vector: zero, never rotated
    if (ia > ib) { const int t = ia; ia = ib; ib = t; }
    double* a = j.z + (size_t)ia * j.r;
    double* b = j.z + (size_t)ib * j.r;
    double al = 0.0, be = 0.0, ga = 0.0;
    for (int f = tid; f < j.r; f += JC_THREADS) {
        const double x = a[f], y = b[f];
        if (LDS) { vec[f] = x; vec[j.r + f] = y; }
        al += x * x; be += y * y; ga += x * y;
    }
    al = wave_sum(al); be = wave_sum(be); ga = wave_sum(ga);
    if ((tid & 63) == 0) { red[tid >> 6] = al; red[4 + (tid >> 6)] = be; red[8 + (tid >> 6)] = ga; }
    __syncthreads();
    al = ((red[0] + red[1]) + red[2]) + red[3];
    be = ((red[4] + red[5]) + red[6]) + red[7];
    ga = ((red[8] + red[9]) + red[10]) + red[11];
    if (!isfinite(al) || !isfinite(be) || !isfinite(ga)) {
        if (tid == 0) atomicAdd(&j.counter[1], 1);
        return;
    }
    const double tol = (double)j.r * 0x1p-53, fl = 0x1p-53 * j.fro2[0], ab = al * be;
    if (!(fabs(ga) > tol * sqrt(ab)) || !(ab > fl * fl)) return;    // orthogonal to working precision, or both inside the noise floor
    const double zeta = (be - al) / (2.0 * ga);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));   // the smaller-angle tangent
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    for (int f = tid; f < j.r; f += JC_THREADS) {                   // each thread reads back the elements it staged itself
        const double x = LDS ? vec[f] : a[f], y = LDS ? vec[j.r + f] : b[f];
        a[f] = c * x - s * y;
        b[f] = s * x + c * y;
    }
    if (tid == 0) atomicAdd(&j.counter[0], 1);
}

// alpha[i] = |z_i|^2, one workgroup per vector
__global__ void __launch_bounds__(256) sq_norms_kernel(const double* z, int r, double* alpha) {
    __shared__ double red[4];
    const double* v = z + (size_t)blockIdx.x * r;
    double s = 0.0;
    for (int f = threadIdx.x; f < r; f += 256) s += v[f] * v[f];
    s = block_sum(s, red);
    if (threadIdx.x == 0) alpha[blockIdx.x] = s;
}

// svals = sqrt(alpha) sorted descending (bitonic over the next power of two, padded with -1), nuclear = their sum in a fixed order
__global__ void __launch_bounds__(256) svals_kernel(const double* alpha, int n, int P, double* svals, double* nuclear) {
    __shared__ double v[JC_MAX_N];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += 256) v[i] = i < n ? sqrt(alpha[i]) : -1.0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int l = i ^ jj;
                if (l > i) {
                    const double x = v[i], y = v[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? x < y : x > y) { v[i] = y; v[l] = x; }
                }
            }
            __syncthreads();
        }
    double s = 0.0;
    for (int i = tid; i < n; i += 256) {
        if (svals) svals[i] = v[i];
        s += v[i];
    }
    s = block_sum(s, red);
    if (tid == 0 && nuclear) nuclear[0] = s;
}

// out: {FD, |mx - my|^2, tr S1, tr S2, ||C||_*, ||C||_F^2}; sc: {dm2, ssq1, ssq2, nuclear, fro2}
__global__ void frechet_final_kernel(const double* sc, int n1, int n2, double* out) {
    if (threadIdx.x || blockIdx.x) return;
    const double t1 = sc[1] / (double)(n1 - 1), t2 = sc[2] / (double)(n2 - 1);
    out[0] = ((sc[0] + t1) + t2) - 2.0 * sc[3];
    out[1] = sc[0]; out[2] = t1; out[3] = t2; out[4] = sc[3]; out[5] = sc[4];
}

// out: {MMD^2, sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum k(x_i, y_j)}
__global__ void kid_final_kernel(const double* sums, int n1, int n2, double* out) {
    if (threadIdx.x || blockIdx.x) return;
    const double a = sums[0] / ((double)n1 * (double)(n1 - 1)), b = sums[1] / ((double)n2 * (double)(n2 - 1));
    const double c = sums[2] / ((double)n1 * (double)n2);
    out[0] = (a + b) - 2.0 * c;
    out[1] = sums[0]; out[2] = sums[1]; out[3] = sums[2];
}

// ------------------------------------------------------------------------------------------------ moment form
// State of a set: n (host), mean [dim], M [dim][dim] = sum (x - mean)(x - mean)^T, full and bit-symmetric.  A batch enters through its
// own centred scatter and Chan's pairwise update: M += Mb + w d d^T, d = mean_b - mean, w = n nb / (n + nb).
struct ScatterArgs {
    const float* x;              // [nb][dim]
    const double *mb, *delta;    // [dim]: the batch's mean; mean_b - mean (zeros for the first batch)
    int nb, dim;                 // workgroup b of cdiv(dim, 32) (cdiv(dim, 32) + 1) / 2 owns tile (ti, tj), tj <= ti, b = ti (ti + 1) / 2 + tj
    double w;
    double* m;                   // [dim][dim] in/out
    int first;                   // store, do not read M
};

// C[f][g] = sum_rows (x[r][f] - mb[f]) (x[r][g] - mb[g]): gram_kernel with the roles turned -- the inner extent is the row index and both
// operands are column blocks of one matrix.  A wave's 32 lanes load 32 neighbouring features of one row (coalesced) and store them
// down a column of the [feature][row] LDS tile: stride GR_LD = 33 doubles, 32 different banks.  The MFMA side reads the tile as
// gram_kernel does.  A diagonal tile stages one operand.  Each tile has one owner, who also writes the mirror: no atomics, M == M^T.
__global__ void __launch_bounds__(GR_THREADS) scatter_kernel(const ScatterArgs g) {
    __shared__ double As[GR_T * GR_LD], Bs[GR_T * GR_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int ti = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    while (ti * (ti + 1) / 2 > (int)blockIdx.x) --ti;
    const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
    const bool diag = ti == tj;
    const int i0 = ti * GR_T, j0 = tj * GR_T;
    const int lr = tid >> 5, lc = tid & 31;                   // this thread stages rows lr + 8 q of a chunk, feature lc of both blocks
    const int fa = i0 + lc, fb = j0 + lc;
    const bool aok = fa < g.dim, bok = fb < g.dim && !diag;
    const double ca = aok ? g.mb[fa] : 0.0, cb = bok ? g.mb[fb] : 0.0;
    double ra[4], rb[4];
    auto load = [&](int r0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + lr + 8 * q;
            const bool rok = r < g.nb;
            ra[q] = (rok && aok) ? (double)g.x[(size_t)r * g.dim + fa] - ca : 0.0;
            rb[q] = (rok && bok) ? (double)g.x[(size_t)r * g.dim + fb] - cb : 0.0;
        }
    };
    const int wi = (w >> 1) * 16, wj = (w & 1) * 16;
    const int ar = (wi + (lane & 15)) * GR_LD + (lane >> 4), br = (wj + (lane & 15)) * GR_LD + (lane >> 4);
    const double* Bp = diag ? As : Bs;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    load(0);
    for (int r0 = 0; r0 < g.nb; r0 += GR_BK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            As[lc * GR_LD + lr + 8 * q] = ra[q];
            if (!diag) Bs[lc * GR_LD + lr + 8 * q] = rb[q];
        }
        __syncthreads();
        if (r0 + GR_BK < g.nb) load(r0 + GR_BK);
#pragma unroll
        for (int kk = 0; kk < GR_BK / 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[ar + 4 * kk], Bp[br + 4 * kk], acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = j0 + wj + (lane & 15);
    if (col >= g.dim) return;
    const double dc = g.delta[col];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = i0 + wi + (lane >> 4) + 4 * reg;
        if (row >= g.dim || (diag && row < col)) continue;     // a diagonal tile: the lower triangle's lanes own both elements
        double v = acc[reg] + g.w * (g.delta[row] * dc);
        if (!g.first) v = g.m[(size_t)row * g.dim + col] + v;
        g.m[(size_t)row * g.dim + col] = v;
        if (row != col) g.m[(size_t)col * g.dim + row] = v;
    }
}

// delta[f] = mean_b[f] - mean[f], mean[f] += frac delta[f]; the first batch: delta = 0, mean = mean_b
__global__ void __launch_bounds__(256) mean_merge_kernel(const double* mean_b, int dim, double frac, int first, double* mean, double* delta) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= dim) return;
    const double d = first ? 0.0 : mean_b[f] - mean[f];
    delta[f] = d;
    mean[f] = first ? mean_b[f] : mean[f] + frac * d;
}

// M_a[f][g] += M_b[f][g] + w delta[f] delta[g] (symmetric in, symmetric out: the product of the deltas commutes); first: M_a = M_b
__global__ void __launch_bounds__(256) scatter_merge_kernel(const double* mb, const double* delta, int dim, double w, int first, double* ma) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)dim * dim) return;
    const int f = (int)(i / dim), gg = (int)(i % dim);
    const double v = mb[i] + w * (delta[f] * delta[gg]);
    ma[i] = first ? mb[i] : ma[i] + v;
}

// z = scale M
__global__ void __launch_bounds__(256) scale_copy_kernel(const double* m, long long count, double scale, double* z) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) z[i] = scale * m[i];
}

// out[0] = scale * sum_f M[f][f], thread t adds f = t, t + 256, ... in order
__global__ void __launch_bounds__(256) trace_kernel(const double* m, int dim, double scale, double* out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int f = threadIdx.x; f < dim; f += 256) s += m[(size_t)f * dim + f];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = scale * s;
}

// f_i = z_i / sqrt(|z_i|) with alpha[i] = |z_i|^2, one workgroup per vector; a zero (or non-finite-norm) row is left as it is
__global__ void __launch_bounds__(256) factor_scale_kernel(double* z, int r, const double* alpha) {
    const double a = alpha[blockIdx.x];
    if (!(a > 0.0) || !isfinite(a)) return;
    const double s = 1.0 / sqrt(sqrt(a));
    double* v = z + (size_t)blockIdx.x * r;
    for (int f = threadIdx.x; f < r; f += 256) v[f] = s * v[f];
}

// out: {FD, |m1 - m2|^2, tr S1, tr S2, ||F1 F2^T||_*, ||F1 F2^T||_F^2}; sc: {dm2, nuclear, fro2}
__global__ void moments_final_kernel(const double* sc, const double* tr1, const double* tr2, double* out) {
    if (threadIdx.x || blockIdx.x) return;
    out[0] = ((sc[0] + tr1[0]) + tr2[0]) - 2.0 * sc[1];
    out[1] = sc[0]; out[2] = tr1[0]; out[3] = tr2[0]; out[4] = sc[1]; out[5] = sc[2];
}

// ------------------------------------------------------------------------------------------------ host side
static inline long long fr_align(long long b) { return (b + 15) / 16 * 16; }
static inline long long fr_tiles(int n1, int n2) { return (long long)cdiv(n1, GR_T) * cdiv(n2, GR_T); }
static inline long long fr_cm_blocks(long long dim) { return (dim + CM_F - 1) / CM_F; }
static inline int fr_pow2(int n) { int p = 2; while (p < n) p <<= 1; return p; }

constexpr long long JC_COUNTER_BYTES = 2 * FC_JACOBI_MAX_SWEEPS * 4 + 16, FR_SCALAR_BYTES = 128;
struct JacobiWs { long long alpha, counters, scalars, total; };     // scalars: {fro2, nuclear}
static JacobiWs jacobi_ws_layout(int n) {
    JacobiWs w = {};
    long long o = 0;
    w.alpha = o; o += fr_align((long long)n * 8);
    w.counters = o; o += fr_align(JC_COUNTER_BYTES);
    w.scalars = o; o += FR_SCALAR_BYTES;
    w.total = o;
    return w;
}
struct FrechetWs { long long mean_a, mean_b, z, part, scalars, jacobi, total; };
static FrechetWs frechet_ws_layout(int ns, int nl, long long dim) {
    FrechetWs w = {};
    long long o = 0;
    w.mean_a = o; o += fr_align(dim * 8);
    w.mean_b = o; o += fr_align(dim * 8);
    w.z = o; o += fr_align((long long)ns * nl * 8);
    const long long parts = fr_tiles(ns, nl) > fr_cm_blocks(dim) ? fr_tiles(ns, nl) : fr_cm_blocks(dim);
    w.part = o; o += fr_align(parts * 8);
    w.scalars = o; o += FR_SCALAR_BYTES;
    w.jacobi = o; o += jacobi_ws_layout(ns).total;
    w.total = o;
    return w;
}

struct MomentsUpdateWs { long long mean_b, delta, part, scalars, total; };
static MomentsUpdateWs moments_update_ws_layout(long long dim) {
    MomentsUpdateWs w = {};
    long long o = 0;
    w.mean_b = o; o += fr_align(dim * 8);
    w.delta = o; o += fr_align(dim * 8);
    w.part = o; o += fr_align(fr_cm_blocks(dim) * 8);
    w.scalars = o; o += FR_SCALAR_BYTES;
    w.total = o;
    return w;
}
struct MomentsDistanceWs { long long g, part, scalars, jacobi, total; };     // scalars: {dm2, nuclear, fro2}
static MomentsDistanceWs moments_distance_ws_layout(int dim) {
    MomentsDistanceWs w = {};
    long long o = 0;
    w.g = o; o += fr_align((long long)dim * dim * 8);
    w.part = o; o += fr_align(fr_tiles(dim, dim) * 8);
    w.scalars = o; o += FR_SCALAR_BYTES;
    w.jacobi = o; o += jacobi_ws_layout(dim).total;
    w.total = o;
    return w;
}

static bool fr_misaligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) != 0; }

template <typename T>
static int gram_launch(const GramArgsT<T>& g, bool reduce, hipStream_t s) {
    const dim3 grid(cdiv(g.n2, GR_T), cdiv(g.n1, GR_T));
    if (reduce) hipLaunchKernelGGL((gram_kernel<true, T>), grid, dim3(GR_THREADS), 0, s, g);
    else hipLaunchKernelGGL((gram_kernel<false, T>), grid, dim3(GR_THREADS), 0, s, g);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

static int moments_launch(const float* x, int n, long long dim, double* mean, double* part, double* ssq_out, hipStream_t s) {
    const long long blocks = fr_cm_blocks(dim);
    hipLaunchKernelGGL(col_moments_kernel, dim3((unsigned)blocks), dim3(CM_F * CM_R), 0, s, x, n, dim, mean, part);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, part, blocks, ssq_out);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// Sweeps over z [n][r] until one sweep rotates nothing, at most FC_JACOBI_MAX_SWEEPS; the host reads one 8-byte word per sweep.
// fro2: ||Z||_F^2 on the device.  Then the sorted norms (svals, may be null) and their sum (nuclear, may be null).
static int jacobi_run(double* z, int n, int r, const double* fro2, char* jws, double* svals, double* nuclear, int* sweeps_out,
                      int* converged_out, long long* launches_out, hipStream_t s) {
    const JacobiWs w = jacobi_ws_layout(n);
    int* counters = reinterpret_cast<int*>(jws + w.counters);
    double* alpha = reinterpret_cast<double*>(jws + w.alpha);
    FC_HIP(hipMemsetAsync(counters, 0, JC_COUNTER_BYTES, s));
    JacobiArgs j = {};
    j.z = z; j.n = n; j.m = n + (n & 1); j.r = r; j.fro2 = fro2;
    const bool lds = r <= FC_JACOBI_LDS_R;
    const size_t lds_bytes = lds ? (size_t)2 * r * 8 : 0;
    int sweeps = 0, converged = 0;
    long long launches = 0;
    for (int sweep = 0; sweep < FC_JACOBI_MAX_SWEEPS; ++sweep) {
        j.counter = counters + 2 * sweep;
        for (int round = 0; round < j.m - 1; ++round) {
            j.round = round;
            if (lds) hipLaunchKernelGGL(jacobi_pair_kernel<true>, dim3(j.m / 2), dim3(JC_THREADS), lds_bytes, s, j);
            else hipLaunchKernelGGL(jacobi_pair_kernel<false>, dim3(j.m / 2), dim3(JC_THREADS), 0, s, j);
            FC_HIP(hipGetLastError());
            ++launches;
        }
        int word[2] = {0, 0};
        FC_HIP(hipMemcpyAsync(word, j.counter, 8, hipMemcpyDeviceToHost, s));
        FC_HIP(hipStreamSynchronize(s));
        sweeps = sweep + 1;
        if (word[1] != 0) break;                                    // a non-finite product: no convergence to wait for
        if (word[0] == 0) { converged = 1; break; }
    }
    hipLaunchKernelGGL(sq_norms_kernel, dim3(n), dim3(256), 0, s, z, r, alpha);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(svals_kernel, dim3(1), dim3(256), 0, s, alpha, n, fr_pow2(n), svals, nuclear);
    FC_HIP(hipGetLastError());
    *sweeps_out = sweeps; *converged_out = converged;
    if (launches_out) *launches_out = launches + 2;
    return FC_OK;
}

static int sets_check(const char* who, const void* x, int n1, const void* y, int n2, long long dim) {
    if (!x || !y) return fail(FC_E_ARG, std::string(who) + ": null argument");
    if (fr_misaligned(x, 4) || fr_misaligned(y, 4)) return fail(FC_E_ARG, std::string(who) + ": a float pointer that is not 4-byte aligned");
    if (dim < 1) return fail(FC_E_SHAPE, std::string(who) + ": dim >= 1");
    if (n1 < 2 || n2 < 2) return fail(FC_E_SHAPE, std::string(who) + ": both sets need at least two samples");
    return FC_OK;
}

}  // namespace fc

using namespace fc;

extern "C" {

int64_t fc_frechet_workspace_bytes(int what, int n1, int n2, int64_t dim) {
    if (n1 < 1 || n2 < 1 || dim < 1 || n1 > FC_GRAM_MAX_ROWS || n2 > FC_GRAM_MAX_ROWS)
        return fail(FC_E_SHAPE, "fc_frechet_workspace_bytes: 1 <= n1, n2 <= 65536 and dim >= 1");
    const int ns = n1 < n2 ? n1 : n2, nl = n1 < n2 ? n2 : n1;
    switch (what) {
    case FC_WS_GRAM: return fr_align(fr_tiles(n1, n2) * 8);
    case FC_WS_MOMENTS: return fr_align(fr_cm_blocks(dim) * 8);
    case FC_WS_JACOBI:
        if (n1 > FC_FRECHET_MAX_SMALL) return fail(FC_E_SHAPE, "fc_frechet_workspace_bytes: at most 4096 vectors");
        return jacobi_ws_layout(n1).total;
    case FC_WS_FRECHET:
        if (ns > FC_FRECHET_MAX_SMALL || nl > FC_FRECHET_MAX_LARGE)
            return fail(FC_E_SHAPE, "fc_frechet_workspace_bytes: min(n1, n2) <= 4096 and max(n1, n2) <= 16384");
        return frechet_ws_layout(ns, nl, dim).total;
    case FC_WS_KID:
        if (nl > FC_FRECHET_MAX_LARGE) return fail(FC_E_SHAPE, "fc_frechet_workspace_bytes: max(n1, n2) <= 16384");
        return fr_align((fr_tiles(n1, n1) + fr_tiles(n2, n2) + fr_tiles(n1, n2)) * 8) + FR_SCALAR_BYTES;
    case FC_WS_MOMENTS_UPDATE:
    case FC_WS_MOMENTS_MERGE:
    case FC_WS_MOMENTS_FACTOR:
    case FC_WS_MOMENTS_DISTANCE:
        if (dim > FC_FRECHET_MAX_SMALL) return fail(FC_E_SHAPE, "fc_frechet_workspace_bytes: the moment form takes dim <= 4096");
        if (what == FC_WS_MOMENTS_UPDATE) return moments_update_ws_layout(dim).total;
        if (what == FC_WS_MOMENTS_MERGE) return fr_align(dim * 8);
        if (what == FC_WS_MOMENTS_FACTOR) return jacobi_ws_layout((int)dim).total;
        return moments_distance_ws_layout((int)dim).total;
    }
    return fail(FC_E_ARG, "fc_frechet_workspace_bytes: unknown workspace kind");
}

int fc_gram_f64(const float* a_dev, int n1, const float* b_dev, int n2, int64_t dim, const double* mean_a_dev, const double* mean_b_dev,
                double scale, double* c_out_dev, double* fro2_out_dev, void* ws_dev, void* stream) {
    if (!a_dev || !b_dev || !c_out_dev || (fro2_out_dev && !ws_dev)) return fail(FC_E_ARG, "fc_gram_f64: null argument");
    if (n1 < 1 || n2 < 1 || dim < 1 || n1 > FC_GRAM_MAX_ROWS || n2 > FC_GRAM_MAX_ROWS)
        return fail(FC_E_SHAPE, "fc_gram_f64: 1 <= n1, n2 <= 65536 and dim >= 1");
    if (fr_misaligned(a_dev, 4) || fr_misaligned(b_dev, 4) || fr_misaligned(mean_a_dev, 8) || fr_misaligned(mean_b_dev, 8) ||
        fr_misaligned(c_out_dev, 8) || fr_misaligned(fro2_out_dev, 8) || fr_misaligned(ws_dev, 8))
        return fail(FC_E_ARG, "fc_gram_f64: a pointer that is not naturally aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    GramArgs g = {};
    g.a = a_dev; g.b = b_dev; g.ma = mean_a_dev; g.mb = mean_b_dev; g.n1 = n1; g.n2 = n2; g.dim = dim; g.scale = scale; g.c = c_out_dev;
    g.part = fro2_out_dev ? static_cast<double*>(ws_dev) : nullptr;
    FC_TRY(gram_launch(g, false, s));
    if (fro2_out_dev) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, g.part, fr_tiles(n1, n2), fro2_out_dev);
        FC_HIP(hipGetLastError());
    }
    return FC_OK;
}

int fc_col_moments(const float* x_dev, int n, int64_t dim, double* mean_out_dev, double* ssq_out_dev, void* ws_dev, void* stream) {
    if (!x_dev || !mean_out_dev || !ssq_out_dev || !ws_dev) return fail(FC_E_ARG, "fc_col_moments: null argument");
    if (n < 1 || n > FC_GRAM_MAX_ROWS || dim < 1) return fail(FC_E_SHAPE, "fc_col_moments: 1 <= n <= 65536 and dim >= 1");
    if (fr_misaligned(x_dev, 4) || fr_misaligned(mean_out_dev, 8) || fr_misaligned(ssq_out_dev, 8) || fr_misaligned(ws_dev, 8))
        return fail(FC_E_ARG, "fc_col_moments: a pointer that is not naturally aligned");
    return moments_launch(x_dev, n, dim, mean_out_dev, static_cast<double*>(ws_dev), ssq_out_dev, static_cast<hipStream_t>(stream));
}

int fc_jacobi_svals(double* z_inout_dev, int n, int r, double* svals_out_dev, double* nuclear_out_dev, void* ws_dev, int* sweeps_out_host,
                    int* converged_out_host, void* stream) {
    if (!z_inout_dev || !svals_out_dev || !ws_dev || !sweeps_out_host || !converged_out_host) return fail(FC_E_ARG, "fc_jacobi_svals: null argument");
    if (n < 1 || n > FC_FRECHET_MAX_SMALL || r < 1) return fail(FC_E_SHAPE, "fc_jacobi_svals: 1 <= n <= 4096 vectors of r >= 1 elements");
    if (fr_misaligned(z_inout_dev, 8) || fr_misaligned(svals_out_dev, 8) || fr_misaligned(nuclear_out_dev, 8) || fr_misaligned(ws_dev, 16))
        return fail(FC_E_ARG, "fc_jacobi_svals: a pointer that is not naturally aligned (the workspace: 16 bytes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(ws_dev);
    const JacobiWs w = jacobi_ws_layout(n);
    double* alpha = reinterpret_cast<double*>(ws + w.alpha);
    double* fro2 = reinterpret_cast<double*>(ws + w.scalars);
    hipLaunchKernelGGL(sq_norms_kernel, dim3(n), dim3(256), 0, s, z_inout_dev, r, alpha);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, alpha, (long long)n, fro2);
    FC_HIP(hipGetLastError());
    return jacobi_run(z_inout_dev, n, r, fro2, ws, svals_out_dev, nuclear_out_dev, sweeps_out_host, converged_out_host, nullptr, s);
}

int fc_frechet_sets(const float* x_dev, int n1, const float* y_dev, int n2, int64_t dim, void* ws_dev, double* out_dev, double* svals_out_dev,
                    int* sweeps_out_host, int* converged_out_host, int64_t* launches_out_host, void* stream) {
    FC_TRY(sets_check("fc_frechet_sets", x_dev, n1, y_dev, n2, dim));
    if (!ws_dev || !out_dev || !sweeps_out_host || !converged_out_host) return fail(FC_E_ARG, "fc_frechet_sets: null argument");
    const bool swap = n2 < n1;                                      // the smaller set first: its rows of C are the vectors to orthogonalise
    const int ns = swap ? n2 : n1, nl = swap ? n1 : n2;
    if (ns > FC_FRECHET_MAX_SMALL || nl > FC_FRECHET_MAX_LARGE)
        return fail(FC_E_SHAPE, "fc_frechet_sets: min(n1, n2) <= 4096 and max(n1, n2) <= 16384");
    if (fr_misaligned(ws_dev, 16) || fr_misaligned(out_dev, 8) || fr_misaligned(svals_out_dev, 8))
        return fail(FC_E_ARG, "fc_frechet_sets: the workspace must be 16-byte aligned, the outputs 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* a = swap ? y_dev : x_dev;
    const float* b = swap ? x_dev : y_dev;
    char* ws = static_cast<char*>(ws_dev);
    const FrechetWs w = frechet_ws_layout(ns, nl, dim);
    double* ma = reinterpret_cast<double*>(ws + w.mean_a);
    double* mb = reinterpret_cast<double*>(ws + w.mean_b);
    double* z = reinterpret_cast<double*>(ws + w.z);
    double* part = reinterpret_cast<double*>(ws + w.part);
    double* sc = reinterpret_cast<double*>(ws + w.scalars);         // {dm2, ssq_a, ssq_b, nuclear, fro2}
    FC_TRY(moments_launch(a, ns, dim, ma, part, sc + 1, s));
    FC_TRY(moments_launch(b, nl, dim, mb, part, sc + 2, s));
    hipLaunchKernelGGL(mean_diff2_kernel, dim3(1), dim3(256), 0, s, ma, mb, (long long)dim, sc);
    FC_HIP(hipGetLastError());
    GramArgs g = {};
    g.a = a; g.b = b; g.ma = ma; g.mb = mb; g.n1 = ns; g.n2 = nl; g.dim = dim; g.c = z; g.part = part;
    g.scale = 1.0 / sqrt((double)(ns - 1) * (double)(nl - 1));
    FC_TRY(gram_launch(g, false, s));
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, part, fr_tiles(ns, nl), sc + 4);
    FC_HIP(hipGetLastError());
    long long launches = 0;
    FC_TRY(jacobi_run(z, ns, nl, sc + 4, ws + w.jacobi, svals_out_dev, sc + 3, sweeps_out_host, converged_out_host, &launches, s));
    hipLaunchKernelGGL(frechet_final_kernel, dim3(1), dim3(64), 0, s, sc, ns, nl, out_dev);
    FC_HIP(hipGetLastError());
    if (launches_out_host) *launches_out_host = launches + 8;
    return FC_OK;
}

int fc_kid_sets(const float* x_dev, int n1, const float* y_dev, int n2, int64_t dim, void* ws_dev, double* out_dev, void* stream) {
    FC_TRY(sets_check("fc_kid_sets", x_dev, n1, y_dev, n2, dim));
    if (!ws_dev || !out_dev) return fail(FC_E_ARG, "fc_kid_sets: null argument");
    if (n1 > FC_FRECHET_MAX_LARGE || n2 > FC_FRECHET_MAX_LARGE) return fail(FC_E_SHAPE, "fc_kid_sets: n1, n2 <= 16384");
    if (fr_misaligned(ws_dev, 16) || fr_misaligned(out_dev, 8)) return fail(FC_E_ARG, "fc_kid_sets: the workspace must be 16-byte aligned, the output 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws_dev);
    const long long t[3] = {fr_tiles(n1, n1), fr_tiles(n2, n2), fr_tiles(n1, n2)};
    double* sums = part + fr_align((t[0] + t[1] + t[2]) * 8) / 8;
    const float* lhs[3] = {x_dev, y_dev, x_dev};
    const float* rhs[3] = {x_dev, y_dev, y_dev};
    const int nl[3] = {n1, n2, n1}, nr[3] = {n1, n2, n2};
    long long off = 0;
    for (int q = 0; q < 3; ++q) {
        GramArgs g = {};
        g.a = lhs[q]; g.b = rhs[q]; g.n1 = nl[q]; g.n2 = nr[q]; g.dim = dim; g.scale = 1.0; g.part = part + off; g.skip_diag = q < 2;
        FC_TRY(gram_launch(g, true, s));
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, part + off, t[q], sums + q);
        FC_HIP(hipGetLastError());
        off += t[q];
    }
    hipLaunchKernelGGL(kid_final_kernel, dim3(1), dim3(64), 0, s, sums, n1, n2, out_dev);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

static int moments_dim_check(const char* who, int64_t dim) {
    if (dim < 1 || dim > FC_FRECHET_MAX_SMALL) return fail(FC_E_SHAPE, std::string(who) + ": 1 <= dim <= 4096");
    return FC_OK;
}

int fc_frechet_moments_update(const float* x_dev, int nb, int dim, int64_t n_before, double* mean_inout_dev, double* m_inout_dev, void* ws_dev,
                              void* stream) {
    if (!x_dev || !mean_inout_dev || !m_inout_dev || !ws_dev) return fail(FC_E_ARG, "fc_frechet_moments_update: null argument");
    FC_TRY(moments_dim_check("fc_frechet_moments_update", dim));
    if (nb < 1 || nb > FC_GRAM_MAX_ROWS || n_before < 0) return fail(FC_E_SHAPE, "fc_frechet_moments_update: 1 <= nb <= 65536 and n_before >= 0");
    if (fr_misaligned(x_dev, 4) || fr_misaligned(mean_inout_dev, 8) || fr_misaligned(m_inout_dev, 8) || fr_misaligned(ws_dev, 16))
        return fail(FC_E_ARG, "fc_frechet_moments_update: a pointer that is not naturally aligned (the workspace: 16 bytes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(ws_dev);
    const MomentsUpdateWs w = moments_update_ws_layout(dim);
    double* mean_b = reinterpret_cast<double*>(ws + w.mean_b);
    double* delta = reinterpret_cast<double*>(ws + w.delta);
    FC_TRY(moments_launch(x_dev, nb, dim, mean_b, reinterpret_cast<double*>(ws + w.part), reinterpret_cast<double*>(ws + w.scalars), s));
    const int first = n_before == 0;
    const double total = (double)n_before + (double)nb;
    hipLaunchKernelGGL(mean_merge_kernel, dim3(cdiv(dim, 256)), dim3(256), 0, s, mean_b, dim, (double)nb / total, first, mean_inout_dev, delta);
    FC_HIP(hipGetLastError());
    ScatterArgs g = {};
    g.x = x_dev; g.mb = mean_b; g.delta = delta; g.nb = nb; g.dim = dim;
    g.w = (double)n_before * (double)nb / total; g.m = m_inout_dev; g.first = first;
    const int tiles = cdiv(dim, GR_T);
    hipLaunchKernelGGL(scatter_kernel, dim3(tiles * (tiles + 1) / 2), dim3(GR_THREADS), 0, s, g);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int fc_frechet_moments_merge(int dim, int64_t n_a, double* mean_a_inout_dev, double* m_a_inout_dev, int64_t n_b, const double* mean_b_dev,
                             const double* m_b_dev, void* ws_dev, void* stream) {
    if (!mean_a_inout_dev || !m_a_inout_dev || !mean_b_dev || !m_b_dev || !ws_dev) return fail(FC_E_ARG, "fc_frechet_moments_merge: null argument");
    FC_TRY(moments_dim_check("fc_frechet_moments_merge", dim));
    if (n_a < 0 || n_b < 1) return fail(FC_E_SHAPE, "fc_frechet_moments_merge: n_a >= 0 and n_b >= 1");
    if (fr_misaligned(mean_a_inout_dev, 8) || fr_misaligned(m_a_inout_dev, 8) || fr_misaligned(mean_b_dev, 8) || fr_misaligned(m_b_dev, 8) ||
        fr_misaligned(ws_dev, 16))
        return fail(FC_E_ARG, "fc_frechet_moments_merge: a pointer that is not naturally aligned (the workspace: 16 bytes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* delta = static_cast<double*>(ws_dev);
    const int first = n_a == 0;
    const double total = (double)n_a + (double)n_b;
    hipLaunchKernelGGL(mean_merge_kernel, dim3(cdiv(dim, 256)), dim3(256), 0, s, mean_b_dev, dim, (double)n_b / total, first, mean_a_inout_dev, delta);
    FC_HIP(hipGetLastError());
    const long long count = (long long)dim * dim;
    hipLaunchKernelGGL(scatter_merge_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, m_b_dev, delta, dim,
                       (double)n_a * (double)n_b / total, first, m_a_inout_dev);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int fc_frechet_moments_factor(int dim, int64_t n, const double* m_dev, double* factor_out_dev, double* evals_out_dev, double* trace_out_dev,
                              void* ws_dev, int* sweeps_out_host, int* converged_out_host, int64_t* launches_out_host, void* stream) {
    if (!m_dev || !factor_out_dev || !evals_out_dev || !trace_out_dev || !ws_dev || !sweeps_out_host || !converged_out_host)
        return fail(FC_E_ARG, "fc_frechet_moments_factor: null argument");
    FC_TRY(moments_dim_check("fc_frechet_moments_factor", dim));
    if (n < 2) return fail(FC_E_SHAPE, "fc_frechet_moments_factor: a covariance needs n >= 2 samples");
    if (fr_misaligned(m_dev, 8) || fr_misaligned(factor_out_dev, 8) || fr_misaligned(evals_out_dev, 8) || fr_misaligned(trace_out_dev, 8) ||
        fr_misaligned(ws_dev, 16))
        return fail(FC_E_ARG, "fc_frechet_moments_factor: a pointer that is not naturally aligned (the workspace: 16 bytes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(ws_dev);
    const JacobiWs w = jacobi_ws_layout(dim);
    double* alpha = reinterpret_cast<double*>(ws + w.alpha);
    double* fro2 = reinterpret_cast<double*>(ws + w.scalars);
    const double scale = 1.0 / (double)(n - 1);
    const long long count = (long long)dim * dim;
    hipLaunchKernelGGL(scale_copy_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, m_dev, count, scale, factor_out_dev);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(trace_kernel, dim3(1), dim3(256), 0, s, m_dev, dim, scale, trace_out_dev);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(sq_norms_kernel, dim3(dim), dim3(256), 0, s, factor_out_dev, dim, alpha);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, alpha, (long long)dim, fro2);
    FC_HIP(hipGetLastError());
    long long launches = 0;
    FC_TRY(jacobi_run(factor_out_dev, dim, dim, fro2, ws, evals_out_dev, nullptr, sweeps_out_host, converged_out_host, &launches, s));
    hipLaunchKernelGGL(factor_scale_kernel, dim3(dim), dim3(256), 0, s, factor_out_dev, dim, alpha);   // alpha: the final norms, jacobi_run's
    FC_HIP(hipGetLastError());
    if (launches_out_host) *launches_out_host = launches + 5;
    return FC_OK;
}

int fc_frechet_moments_distance(int dim, const double* mean1_dev, const double* factor1_dev, const double* trace1_dev, const double* mean2_dev,
                                const double* factor2_dev, const double* trace2_dev, void* ws_dev, double* out_dev, double* svals_out_dev,
                                int* sweeps_out_host, int* converged_out_host, int64_t* launches_out_host, void* stream) {
    if (!mean1_dev || !factor1_dev || !trace1_dev || !mean2_dev || !factor2_dev || !trace2_dev || !ws_dev || !out_dev || !sweeps_out_host ||
        !converged_out_host)
        return fail(FC_E_ARG, "fc_frechet_moments_distance: null argument");
    FC_TRY(moments_dim_check("fc_frechet_moments_distance", dim));
    if (fr_misaligned(mean1_dev, 8) || fr_misaligned(factor1_dev, 8) || fr_misaligned(trace1_dev, 8) || fr_misaligned(mean2_dev, 8) ||
        fr_misaligned(factor2_dev, 8) || fr_misaligned(trace2_dev, 8) || fr_misaligned(out_dev, 8) || fr_misaligned(svals_out_dev, 8) ||
        fr_misaligned(ws_dev, 16))
        return fail(FC_E_ARG, "fc_frechet_moments_distance: a pointer that is not naturally aligned (the workspace: 16 bytes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(ws_dev);
    const MomentsDistanceWs w = moments_distance_ws_layout(dim);
    double* z = reinterpret_cast<double*>(ws + w.g);
    double* part = reinterpret_cast<double*>(ws + w.part);
    double* sc = reinterpret_cast<double*>(ws + w.scalars);         // {dm2, nuclear, fro2}
    hipLaunchKernelGGL(mean_diff2_kernel, dim3(1), dim3(256), 0, s, mean1_dev, mean2_dev, (long long)dim, sc);
    FC_HIP(hipGetLastError());
    GramArgsT<double> g = {};
    g.a = factor1_dev; g.b = factor2_dev; g.n1 = dim; g.n2 = dim; g.dim = dim; g.scale = 1.0; g.c = z; g.part = part;
    FC_TRY(gram_launch(g, false, s));
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, part, fr_tiles(dim, dim), sc + 2);
    FC_HIP(hipGetLastError());
    long long launches = 0;
    FC_TRY(jacobi_run(z, dim, dim, sc + 2, ws + w.jacobi, svals_out_dev, sc + 1, sweeps_out_host, converged_out_host, &launches, s));
    hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(64), 0, s, sc, trace1_dev, trace2_dev, out_dev);
    FC_HIP(hipGetLastError());
    if (launches_out_host) *launches_out_host = launches + 4;
    return FC_OK;
}

}  // extern "C"
