// Exact k nearest neighbours and ball counts between fp32 row sets ("Nearest neighbours").
//
//   d2(a, b) = sum_f (a_f - b_f)^2 by direct differences (the stance of ot.hip), ONE fp32 accumulator per pair that starts at +0 and
//   takes the features in ascending order, acc = fmaf(a_f - b_f, a_f - b_f, acc).  (a - b) and (b - a) differ in sign only and the
//   padding of a feature tail adds fmaf(0, 0, acc) = acc, so d2 is a function of the two vectors alone: the same bits whichever of the
//   two is the query and whichever tile, chunk, batch or call the pair falls in.  A non-finite d2 is stored as FLT_MAX (ot_finite).
//   Neighbours are ordered by (d2, global reference index), so a tie goes to the lower index and every result is unique.
//
// knn_tile_kernel: a workgroup of 256 threads owns a 64 x 128 tile of (query, reference) pairs, 8 x 4 pairs per thread: thread
// (tq, tn) = (tid / 32, tid % 32) has queries 8 tq .. 8 tq + 7 and references tn, tn + 32, tn + 64, tn + 96 of the tile.  Feature chunks
// of 32 go through LDS rows padded to 36 floats and come back as 16-byte reads: per four features a thread reads 12 float4 for 128
// pair-elements, which keeps the tile below the LDS rate (a 4 x 4 block would read 8 float4 for 64).  The next chunk's global loads are in
// flight while the current one is used.  The two members of a reference pair (tn + 64 h, tn + 64 h + 32) share one packed subtract and
// one packed fma.  The tile's d2 never goes to memory:
//   SELECT: it goes to LDS, and one wave per query row sorts the row's 128 keys {d2 bits, index in tile} (bitonic, two keys per lane)
//           after dropping everything that is not below the running list's k-th entry -- a row with no such key costs two ballots --
//           and writes its k smallest to the call's candidate lists [query][tile][k] with their number;
//   BALL:   each thread compares its pairs with the references' radii, the 32 lanes of a query row add up and one integer atomic per
//           (query, tile) with a non-zero count goes to memory.
// knn_merge_kernel: one wave per (query, group of lists) folds sorted lists of at most k entries into one: the running list is one entry
// per lane, the next list arrives reversed, the lane-wise minimum is the 64 smallest of both as a bitonic sequence and six compare-exchange
// steps sort it.  Above 16 tiles a first launch folds groups of 16 tiles and a second one the groups and the caller's running list.
//
// Every loop is bounded by its arguments, no workgroup waits for another, nothing is allocated and nothing is read back.
#include <float.h>

#include "common.h"

namespace fc {

constexpr int KNN_TQ = 64, KNN_TN = 128, KNN_KC = 32, KNN_LD = KNN_KC + 4, KNN_THREADS = 256;
constexpr int KNN_RQ = 8;                      // queries per thread; references per thread: 4 (two packed pairs)
constexpr int KNN_MAX_K = 64;
constexpr int KNN_GROUP = 16;                  // lists one first-level merge wave folds
constexpr int KNN_MAX_TILES = 1024;            // reference tiles per pass: at most 64 groups for the second level
constexpr long long KNN_CAND_BYTES = 64ll << 20;   // candidate lists of one pass stay below this (but one tile always goes)
constexpr int KNN_LDS_FLOATS = KNN_TQ * KNN_TN;    // the d2 tile (8192 floats) covers the staging rows (192 * 36 = 6912)

typedef float knn_f2 __attribute__((ext_vector_type(2)));

struct KnnTile {
    const float* q; const float* ref;
    int n_query; long long n_ref; long long dim;      // n_ref: rows of `ref` in this call
    long long first_index;                            // global index of ref row 0
    const long long* query_ids;                       // or null
    long long tile0; int n_qtiles;                    // first reference tile of this pass; workgroup = qt + n_qtiles * (tile - tile0)
    // SELECT
    int k; int tiles;                                 // lists per query in this pass
    const float* best_d2; const long long* best_idx;  // the running lists [n_query][k]
    float* cand_d2; long long* cand_idx; int* cand_cnt;
    // BALL
    const float* radius2; int* counts;
};

template <bool VEC>
__device__ __forceinline__ float4 knn_load4(const float* base, bool row_ok, long long row, long long dim, long long f) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok) return v;
    const float* p = base + (size_t)row * (size_t)dim + f;
    if (VEC) {
        if (f < dim) v = *reinterpret_cast<const float4*>(p);     // dim % 4 == 0 and f % 4 == 0: all four or none
    } else {
        if (f < dim) v.x = p[0];
        if (f + 1 < dim) v.y = p[1];
        if (f + 2 < dim) v.z = p[2];
        if (f + 3 < dim) v.w = p[3];
    }
    return v;
}

__device__ __forceinline__ unsigned long long knn_shfl_xor64(unsigned long long v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}

template <bool VEC, bool BALL>
__global__ void __launch_bounds__(KNN_THREADS) knn_tile_kernel(const KnnTile a) {
    __shared__ __attribute__((aligned(16))) float smem[KNN_LDS_FLOATS];
    float* sq = smem;                       // [64][36]
    float* sr = smem + KNN_TQ * KNN_LD;     // [128][36]
    const int tid = threadIdx.x, tn = tid & 31, tq = tid >> 5;
    const int qt = blockIdx.x % a.n_qtiles;
    const long long tile = a.tile0 + blockIdx.x / a.n_qtiles;
    const int q0 = qt * KNN_TQ;
    const long long r0 = tile * KNN_TN;     // row of `ref`

    // staging: element e = tid + 256 u is float4 (e & 7) of row (e >> 3); u < 2 for the queries, u < 4 for the references
    float4 gq[2], gr[4];
    auto fetch = [&](long long k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + KNN_THREADS * u, row = e >> 3;
            gq[u] = knn_load4<VEC>(a.q, q0 + row < a.n_query, q0 + row, a.dim, k0 + 4 * (e & 7));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + KNN_THREADS * u, row = e >> 3;
            gr[u] = knn_load4<VEC>(a.ref, r0 + row < a.n_ref, r0 + row, a.dim, k0 + 4 * (e & 7));
        }
    };

    knn_f2 acc[KNN_RQ][2];
#pragma unroll
    for (int i = 0; i < KNN_RQ; ++i) { acc[i][0] = (knn_f2){0.f, 0.f}; acc[i][1] = (knn_f2){0.f, 0.f}; }

    fetch(0);
    for (long long k0 = 0; k0 < a.dim; k0 += KNN_KC) {
        __syncthreads();                    // the previous chunk has been used
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + KNN_THREADS * u;
            *reinterpret_cast<float4*>(sq + (e >> 3) * KNN_LD + 4 * (e & 7)) = gq[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + KNN_THREADS * u;
            *reinterpret_cast<float4*>(sr + (e >> 3) * KNN_LD + 4 * (e & 7)) = gr[u];
        }
        __syncthreads();
        if (k0 + KNN_KC < a.dim) fetch(k0 + KNN_KC);
#pragma unroll 2
        for (int c = 0; c < KNN_KC; c += 4) {
            float4 qv[KNN_RQ], rv[4];
#pragma unroll
            for (int i = 0; i < KNN_RQ; ++i) qv[i] = *reinterpret_cast<const float4*>(sq + (tq * KNN_RQ + i) * KNN_LD + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) rv[j] = *reinterpret_cast<const float4*>(sr + (tn + 32 * j) * KNN_LD + c);
            // features in ascending order for every pair: x, y, z, w of this float4
#define KNN_STEP(m)                                                                              \
    _Pragma("unroll") for (int i = 0; i < KNN_RQ; ++i) {                                         \
        const knn_f2 qq = (knn_f2){qv[i].m, qv[i].m};                                            \
        const knn_f2 d0 = qq - (knn_f2){rv[0].m, rv[1].m}, d1 = qq - (knn_f2){rv[2].m, rv[3].m}; \
        acc[i][0] = __builtin_elementwise_fma(d0, d0, acc[i][0]);                                \
        acc[i][1] = __builtin_elementwise_fma(d1, d1, acc[i][1]);                                \
    }
            KNN_STEP(x) KNN_STEP(y) KNN_STEP(z) KNN_STEP(w)
#undef KNN_STEP
        }
    }

    if (BALL) {
        float rad[4];
        bool ok[4];
        long long gi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long r = r0 + tn + 32 * j;
            ok[j] = r < a.n_ref;
            gi[j] = a.first_index + r;
            rad[j] = ok[j] ? a.radius2[r] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < KNN_RQ; ++i) {
            const int q = q0 + tq * KNN_RQ + i;                        // the same for the 32 lanes that reduce together
            const long long ex = (a.query_ids && q < a.n_query) ? a.query_ids[q] : -1;
            const float d4[4] = {acc[i][0][0], acc[i][0][1], acc[i][1][0], acc[i][1][1]};
            int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) c += (ok[j] && (!a.query_ids || gi[j] != ex) && ot_finite(d4[j]) <= rad[j]) ? 1 : 0;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o);
            if (tn == 0 && q < a.n_query && c > 0) atomicAdd(a.counts + q, c);
        }
        return;
    }

    // ---- selection ----
    __syncthreads();                        // the staging rows have been used: the d2 tile takes their place
#pragma unroll
    for (int i = 0; i < KNN_RQ; ++i) {
        float* row = smem + (tq * KNN_RQ + i) * KNN_TN + tn;
        row[0] = ot_finite(acc[i][0][0]);
        row[32] = ot_finite(acc[i][0][1]);
        row[64] = ot_finite(acc[i][1][0]);
        row[96] = ot_finite(acc[i][1][1]);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int ql = wave * 16; ql < wave * 16 + 16; ++ql) {             // wave-uniform
        const int q = q0 + ql;
        if (q >= a.n_query) break;
        const float kd2 = a.best_d2[(size_t)q * a.k + a.k - 1];
        const long long kidx = a.best_idx[(size_t)q * a.k + a.k - 1];
        const bool open = kidx < 0;                                    // the running list still has an empty slot: everything enters
        const long long ex = a.query_ids ? a.query_ids[q] : -1;
        unsigned long long key[2];
        int npass = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int l = lane + 64 * s;
            const float d = smem[ql * KNN_TN + l];
            const long long r = r0 + l, g = a.first_index + r;
            const bool pass = r < a.n_ref && (!a.query_ids || g != ex) && (open || d < kd2 || (d == kd2 && g < kidx));
            key[s] = pass ? (((unsigned long long)__float_as_uint(d) << 32) | (unsigned)l) : ~0ull;
            npass += __popcll(__ballot(pass));
        }
        int* cnt = a.cand_cnt + (size_t)q * a.tiles + (tile - a.tile0);
        if (npass == 0) {
            if (lane == 0) *cnt = 0;
            continue;
        }
        // bitonic sort of the 128 keys, element n = 64 s + lane, ascending
#pragma unroll
        for (int kk = 2; kk <= 128; kk <<= 1) {
#pragma unroll
            for (int j = kk >> 1; j > 0; j >>= 1) {
                if (j == 64) {
                    const unsigned long long lo = key[0] < key[1] ? key[0] : key[1], hi = key[0] < key[1] ? key[1] : key[0];
                    key[0] = lo; key[1] = hi;
                } else {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int n = lane + 64 * s;
                        const unsigned long long o = knn_shfl_xor64(key[s], j);
                        const bool up = (n & kk) == 0, low = (n & j) == 0;
                        const bool take_min = up == low;
                        key[s] = ((o < key[s]) == take_min) ? o : key[s];
                    }
                }
            }
        }
        const int m = npass < a.k ? npass : a.k;
        if (lane < m) {
            const size_t o = ((size_t)q * a.tiles + (tile - a.tile0)) * a.k + lane;
            a.cand_d2[o] = __uint_as_float((unsigned)(key[0] >> 32));
            a.cand_idx[o] = a.first_index + r0 + (long long)(key[0] & 0x7f);
        }
        if (lane == 0) *cnt = m;
    }
}

// An entry in a lane: d2 as its bit pattern (non-negative floats order as unsigned integers) and the global index; an empty slot
// (+inf, -1) travels as (inf bits, INT64_MAX) so that it sorts behind everything real.
struct KnnEnt { unsigned d; long long i; };
__device__ __forceinline__ bool knn_less(const KnnEnt& x, const KnnEnt& y) { return x.d < y.d || (x.d == y.d && x.i < y.i); }
__device__ __forceinline__ KnnEnt knn_shfl(const KnnEnt& x, int src) {
    KnnEnt r;
    r.d = __shfl(x.d, src);
    const unsigned lo = __shfl((unsigned)x.i, src), hi = __shfl((unsigned)((unsigned long long)x.i >> 32), src);
    r.i = (long long)(((unsigned long long)hi << 32) | lo);
    return r;
}
constexpr unsigned KNN_INF_BITS = 0x7f800000u;
constexpr long long KNN_I64_MAX = 0x7fffffffffffffffll;

struct KnnMerge {
    const float* src_d2; const long long* src_idx; const int* src_cnt;   // [n_query][n_src][k], [n_query][n_src]
    int n_src, group, n_groups;
    float* run_d2; long long* run_idx;           // the caller's running lists, merged in place (second level) or null (first level)
    float* dst_d2; long long* dst_idx; int* dst_cnt;   // first level: [n_query][n_groups][k] and the numbers of entries
    int n_query, k;
};

// grid (ceil(n_query / 4), n_groups), 256 threads: wave w of workgroup x folds group y of query 4 x + w
__global__ void __launch_bounds__(256) knn_merge_kernel(const KnnMerge a) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6), g = blockIdx.y;
    if (q >= a.n_query) return;                  // wave-uniform
    KnnEnt cur = {KNN_INF_BITS, KNN_I64_MAX};
    if (a.run_d2 && lane < a.k) {
        const long long i = a.run_idx[(size_t)q * a.k + lane];
        if (i >= 0) { cur.d = __float_as_uint(a.run_d2[(size_t)q * a.k + lane]); cur.i = i; }
    }
    const int t0 = g * a.group, t1 = t0 + a.group < a.n_src ? t0 + a.group : a.n_src;
    for (int t = t0; t < t1; t += 4) {
        KnnEnt nx[4];
        int c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = t + u < t1 ? a.src_cnt[(size_t)q * a.n_src + t + u] : 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {            // the four lists' loads leave together
            nx[u].d = KNN_INF_BITS; nx[u].i = KNN_I64_MAX;
            if (lane < c[u]) {
                const size_t o = ((size_t)q * a.n_src + t + u) * a.k + lane;
                nx[u].d = __float_as_uint(a.src_d2[o]);
                nx[u].i = a.src_idx[o];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c[u] == 0) continue;             // wave-uniform
            const KnnEnt rev = knn_shfl(nx[u], 63 - lane);
            if (knn_less(rev, cur)) cur = rev;   // the 64 smallest of both lists, bitonic
#pragma unroll
            for (int j = 32; j > 0; j >>= 1) {
                const KnnEnt o = knn_shfl(cur, lane ^ j);
                const bool take_min = (lane & j) == 0;
                if (knn_less(o, cur) == take_min) cur = o;
            }
        }
    }
    const bool real = cur.i != KNN_I64_MAX;
    if (a.run_d2) {
        if (lane < a.k) {
            a.run_d2[(size_t)q * a.k + lane] = real ? __uint_as_float(cur.d) : INFINITY;
            a.run_idx[(size_t)q * a.k + lane] = real ? cur.i : -1;
        }
    } else {
        const int n = __popcll(__ballot(real && lane < a.k));
        if (real && lane < a.k) {
            const size_t o = ((size_t)q * a.n_groups + g) * a.k + lane;
            a.dst_d2[o] = __uint_as_float(cur.d);
            a.dst_idx[o] = cur.i;
        }
        if (lane == 0) a.dst_cnt[(size_t)q * a.n_groups + g] = n;
    }
}

static inline long long knn_align16(long long b) { return (b + 15) / 16 * 16; }

// reference tiles one pass takes: bounded by the candidate bytes, the second level's width and the grid
static int knn_tiles_per_pass(int n_query, long long n_ref, int k) {
    const long long ntiles = (n_ref + KNN_TN - 1) / KNN_TN;
    const long long n_qtiles = ((long long)n_query + KNN_TQ - 1) / KNN_TQ;
    long long per = KNN_CAND_BYTES / ((long long)n_query * k * 12);
    if (per > KNN_MAX_TILES) per = KNN_MAX_TILES;
    if (per > (1ll << 30) / n_qtiles) per = (1ll << 30) / n_qtiles;
    if (per > ntiles) per = ntiles;
    return per < 1 ? 1 : (int)per;
}

struct KnnWs { long long cand_d2, cand_idx, cand_cnt, grp_d2, grp_idx, grp_cnt, total; int per, groups; };
static KnnWs knn_ws_layout(int n_query, long long n_ref, int k) {
    KnnWs w = {};
    w.per = knn_tiles_per_pass(n_query, n_ref, k);
    w.groups = w.per > KNN_GROUP ? cdiv(w.per, KNN_GROUP) : 0;
    const long long lists = (long long)n_query * w.per, glists = (long long)n_query * w.groups;
    long long o = 0;
    w.cand_idx = o; o += knn_align16(lists * k * 8);
    w.cand_d2 = o; o += knn_align16(lists * k * 4);
    w.cand_cnt = o; o += knn_align16(lists * 4);
    w.grp_idx = o; o += knn_align16(glists * k * 8);
    w.grp_d2 = o; o += knn_align16(glists * k * 4);
    w.grp_cnt = o; o += knn_align16(glists * 4);
    w.total = o < 16 ? 16 : o;
    return w;
}

static int knn_check(const char* who, const void* q, int n_query, const void* ref, long long n_ref, long long dim, long long first_index,
                     const void* query_ids) {
    if (!q || !ref) return fail(FC_E_ARG, std::string(who) + ": null argument");
    if (n_query < 1 || n_query > (1 << 30) || n_ref < 0 || dim < 1)
        return fail(FC_E_SHAPE, std::string(who) + ": 1 <= n_query <= 2^30, n_ref >= 0 and dim >= 1");
    if (first_index < 0 || first_index > KNN_I64_MAX - n_ref - 1) return fail(FC_E_SHAPE, std::string(who) + ": first_index + n_ref must be an int64 >= 0");
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(ref)) & 3) return fail(FC_E_ARG, std::string(who) + ": a float pointer that is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(query_ids) & 7) return fail(FC_E_ARG, std::string(who) + ": query_ids is not 8-byte aligned");
    return FC_OK;
}

static inline bool knn_vec_ok(const void* q, const void* ref, long long dim) {
    return dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(ref)) & 15) == 0;
}

}  // namespace fc

using namespace fc;

extern "C" {

int64_t fc_knn_workspace_bytes(int n_query, int64_t n_ref, int k) {
    if (n_query < 1 || n_query > (1 << 30) || n_ref < 0 || k < 1 || k > KNN_MAX_K)
        return fail(FC_E_SHAPE, "fc_knn_workspace_bytes: 1 <= n_query <= 2^30, n_ref >= 0 and 1 <= k <= 64");
    return knn_ws_layout(n_query, n_ref, k).total;
}

int fc_knn_update(const float* q_dev, int n_query, const float* ref_dev, int64_t n_ref, int64_t dim, int k, int64_t first_index,
                  const int64_t* query_ids_dev, float* best_d2_inout_dev, int64_t* best_idx_inout_dev, void* ws_dev, void* stream) {
    FC_TRY(knn_check("fc_knn_update", q_dev, n_query, ref_dev, n_ref, dim, first_index, query_ids_dev));
    if (!best_d2_inout_dev || !best_idx_inout_dev || !ws_dev) return fail(FC_E_ARG, "fc_knn_update: null argument");
    if (k < 1 || k > KNN_MAX_K) return fail(FC_E_SHAPE, "fc_knn_update: 1 <= k <= 64");
    if ((reinterpret_cast<uintptr_t>(best_d2_inout_dev) & 3) || (reinterpret_cast<uintptr_t>(best_idx_inout_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(ws_dev) & 15))
        return fail(FC_E_ARG, "fc_knn_update: the running lists must be naturally aligned and the workspace 16-byte aligned");
    if (n_ref == 0) return FC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const KnnWs w = knn_ws_layout(n_query, n_ref, k);
    char* ws = static_cast<char*>(ws_dev);
    const long long ntiles = (n_ref + KNN_TN - 1) / KNN_TN;
    const bool vec = knn_vec_ok(q_dev, ref_dev, dim);
    KnnTile t = {};
    t.q = q_dev; t.ref = ref_dev; t.n_query = n_query; t.n_ref = n_ref; t.dim = dim; t.first_index = first_index;
    t.query_ids = reinterpret_cast<const long long*>(query_ids_dev);
    t.n_qtiles = cdiv(n_query, KNN_TQ);
    t.k = k; t.best_d2 = best_d2_inout_dev; t.best_idx = reinterpret_cast<const long long*>(best_idx_inout_dev);
    t.cand_d2 = reinterpret_cast<float*>(ws + w.cand_d2); t.cand_idx = reinterpret_cast<long long*>(ws + w.cand_idx);
    t.cand_cnt = reinterpret_cast<int*>(ws + w.cand_cnt);
    for (long long tile0 = 0; tile0 < ntiles; tile0 += w.per) {      // a later pass sees the lists the earlier ones tightened
        const int tiles = (int)(ntiles - tile0 < w.per ? ntiles - tile0 : w.per);
        t.tile0 = tile0; t.tiles = tiles;
        const dim3 grid((unsigned)(t.n_qtiles * tiles));
        if (vec) hipLaunchKernelGGL((knn_tile_kernel<true, false>), grid, dim3(KNN_THREADS), 0, s, t);
        else hipLaunchKernelGGL((knn_tile_kernel<false, false>), grid, dim3(KNN_THREADS), 0, s, t);
        FC_HIP(hipGetLastError());
        KnnMerge m = {};
        m.n_query = n_query; m.k = k;
        m.src_d2 = t.cand_d2; m.src_idx = t.cand_idx; m.src_cnt = t.cand_cnt; m.n_src = tiles;
        if (tiles > KNN_GROUP) {
            m.group = KNN_GROUP; m.n_groups = cdiv(tiles, KNN_GROUP);
            m.dst_d2 = reinterpret_cast<float*>(ws + w.grp_d2); m.dst_idx = reinterpret_cast<long long*>(ws + w.grp_idx);
            m.dst_cnt = reinterpret_cast<int*>(ws + w.grp_cnt);
            hipLaunchKernelGGL(knn_merge_kernel, dim3(cdiv(n_query, 4), m.n_groups), dim3(256), 0, s, m);
            FC_HIP(hipGetLastError());
            m.src_d2 = m.dst_d2; m.src_idx = m.dst_idx; m.src_cnt = m.dst_cnt; m.n_src = m.n_groups;
            m.dst_d2 = nullptr; m.dst_idx = nullptr; m.dst_cnt = nullptr;
        }
        m.group = m.n_src; m.n_groups = 1;
        m.run_d2 = best_d2_inout_dev; m.run_idx = reinterpret_cast<long long*>(best_idx_inout_dev);
        hipLaunchKernelGGL(knn_merge_kernel, dim3(cdiv(n_query, 4), 1), dim3(256), 0, s, m);
        FC_HIP(hipGetLastError());
    }
    return FC_OK;
}

int fc_knn_ball_counts(const float* q_dev, int n_query, const float* ref_dev, int64_t n_ref, int64_t dim, const float* radius2_dev,
                       int64_t first_index, const int64_t* query_ids_dev, int32_t* counts_inout_dev, void* stream) {
    FC_TRY(knn_check("fc_knn_ball_counts", q_dev, n_query, ref_dev, n_ref, dim, first_index, query_ids_dev));
    if (!radius2_dev || !counts_inout_dev) return fail(FC_E_ARG, "fc_knn_ball_counts: null argument");
    if ((reinterpret_cast<uintptr_t>(radius2_dev) | reinterpret_cast<uintptr_t>(counts_inout_dev)) & 3)
        return fail(FC_E_ARG, "fc_knn_ball_counts: radius2 / counts not 4-byte aligned");
    if (n_ref == 0) return FC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long ntiles = (n_ref + KNN_TN - 1) / KNN_TN;
    const bool vec = knn_vec_ok(q_dev, ref_dev, dim);
    KnnTile t = {};
    t.q = q_dev; t.ref = ref_dev; t.n_query = n_query; t.n_ref = n_ref; t.dim = dim; t.first_index = first_index;
    t.query_ids = reinterpret_cast<const long long*>(query_ids_dev);
    t.n_qtiles = cdiv(n_query, KNN_TQ);
    t.radius2 = radius2_dev; t.counts = counts_inout_dev;
    const long long per = (1ll << 30) / t.n_qtiles;
    for (long long tile0 = 0; tile0 < ntiles; tile0 += per) {
        const long long tiles = ntiles - tile0 < per ? ntiles - tile0 : per;
        t.tile0 = tile0;
        const dim3 grid((unsigned)(t.n_qtiles * tiles));
        if (vec) hipLaunchKernelGGL((knn_tile_kernel<true, true>), grid, dim3(KNN_THREADS), 0, s, t);
        else hipLaunchKernelGGL((knn_tile_kernel<false, true>), grid, dim3(KNN_THREADS), 0, s, t);
        FC_HIP(hipGetLastError());
    }
    return FC_OK;
}

}  // extern "C"
