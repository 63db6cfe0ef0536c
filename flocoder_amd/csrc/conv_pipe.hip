// Producer/consumer implicit-GEMM convolution (the fast path; same contract and epilogue as conv_igemm.hip).
//
// Why: in the synchronous kernel one wave per SIMD does everything in series -- issue loads, wait, write LDS, barrier,
// MFMA with exposed LDS latency -- and co-resident workgroups march in lockstep, so the matrix pipe idles most of the
// time (in-kernel stamps: 128x32 tile 17.8 us for 3.8 us of MFMA; 32x32xK4 tile 30 % MFMA efficiency inside the chunk
// loop; profiles/r01_a_*).  Here a workgroup is 8 wave64 with fixed roles:
//
//   waves 0-3  CONSUMERS  own the accumulators; per Cin chunk they run the fully unrolled tap x k MFMA sequence on the
//                         stage that is ready and touch global memory only in the epilogue;
//   waves 4-7  LOADERS    fill the other stage: the weight slab [taps][CC][BN] (+ fused res_conv slab) by LDS-DMA
//                         (global_load_lds_dwordx4, 1 KiB per wave instruction, per-lane SOURCE address, out-of-range
//                         lanes read a 16-byte zero block), the input window through registers (all loads of a thread
//                         issued back to back, then GroupNorm/FiLM/SiLU applied on the way into LDS).
//
// One barrier per chunk hands stages over.  Each SIMD holds one consumer and one loader wave, so MFMA issue and the
// VALU/VMEM work of staging overlap inside a workgroup instead of relying on a lucky phase shift between workgroups.
// A loader thread's patch elements are the same pixels for every chunk (only the channel base moves): their source
// offsets live in registers and the per-(sample, channel) affine table is built once for all Cin.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>
#include "conv_dev.h"
#include "stats_dev.h"

namespace fc {

typedef __attribute__((address_space(3))) void* lptr_t;

// One LDS-DMA wave instruction: 64 lanes x 16 B from per-lane global addresses to lds_dst + lane*16 (wave-uniform base in
// M0).  Inline asm on purpose (cdna_hip_programming.md 5.7): hipcc then keeps these out of its vmcnt bookkeeping, so the
// waits it inserts for the loaders' ordinary register loads do not drain a slab that was issued for a LATER stage; we
// count them by hand (explicit vmcnt(0) before a stage is handed over).  M0 is saved/restored inside the statement.
// (the destination travels as an LDS byte address, not as a generic pointer: casting a generic pointer back to LDS at every site made
// hipcc 7.2 emit an illegal aperture test -- "V_CMP_NE_U32 0, $src_shared_base" -- in some instantiations)
__device__ __forceinline__ void lds_dma16(const float* gsrc, unsigned lds_byte) {
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_byte);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}
typedef float f32x4 __attribute__((ext_vector_type(4)));
// Register load the compiler does not count either (same reason): 16 B per lane; the caller waits with wait_vmcnt().
__device__ __forceinline__ void hidden_load16(f32x4& dst, const float* gsrc) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(gsrc) : "memory");
}
// s_waitcnt vmcnt(n) for a run-time n (the instruction takes an immediate).  vmcnt counts loads and LDS-DMA together in
// issue order, so "all but my n youngest" = everything issued before the slab that is allowed to stay in flight.
__device__ __forceinline__ void wait_vmcnt(int n) {
    // s_waitcnt ignores EXEC, so the selection must be a SCALAR branch: readfirstlane makes n provably wave-uniform
    switch (__builtin_amdgcn_readfirstlane(n)) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
        case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
        case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
        case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
        case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
        case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
        case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
        case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;   // more pieces than cases: drain (correct, just no lookahead)
    }
    __builtin_amdgcn_sched_barrier(0);   // nothing that reads the hidden loads' registers may move above the wait
}
__device__ __forceinline__ void loader_handover() {   // LDS stores of this wave visible, then the workgroup barrier; no vmcnt drain
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// NL = loader waves (4 or 8).  The small-M tiles stream a whole weight slab per 32 or 64 output rows: with four loader waves the
// slab's LDS-DMA issue (~190 cycles per 1 KB piece per wave) took 1.65x the consumers' MFMA time per chunk and the consumers sat
// at the chunk barrier half of the time (profiles/r01_c_stamps.txt); eight loader waves halve the issue time per wave.
// PREC = 1: split-bf16 arithmetic (round 3, codec decoders on request -- never the U-Net, never a default): every fp32 operand x is taken as
// hi + lo with hi = bf16(x), lo = bf16(x - hi), and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 (fp32 accumulation; the
// dropped lo*lo term is 2^-16 relative).  Three MFMAs of 32 cycles cover sixteen channels where the exact-fp32 pipe needs eight of 64: 5.3x
// the matrix rate.  Nobody splits inside the accumulator waves' loop: the weights are split once, when the parameters are packed (PACK_CONV_B3,
// ConvArgs::w_b3) and reach LDS by the same LDS-DMA pieces as the fp32 slab; the window is split by the staging waves on its way into LDS
// (a pixel is read by up to nine taps).  The accumulator waves read 16-byte hi / lo operands and issue MFMAs.  The epilogue is the fp32 kernel's.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// four fp32 values -> their bf16 hi parts and lo parts, packed two per dword (channel order kept)
__device__ __forceinline__ void split_bf16x4(const f32x4& x, uint2& hi, uint2& lo) {
    union { bf16x2_t p; unsigned u; } H0, H1, L0, L1;
    f32x2_t a; a[0] = x.x; a[1] = x.y;
    f32x2_t b; b[0] = x.z; b[1] = x.w;
    H0.p = __builtin_convertvector(a, bf16x2_t);
    H1.p = __builtin_convertvector(b, bf16x2_t);
    f32x2_t ra; ra[0] = x.x - __uint_as_float(H0.u << 16); ra[1] = x.y - __uint_as_float(H0.u & 0xffff0000u);
    f32x2_t rb; rb[0] = x.z - __uint_as_float(H1.u << 16); rb[1] = x.w - __uint_as_float(H1.u & 0xffff0000u);
    L0.p = __builtin_convertvector(ra, bf16x2_t);
    L1.p = __builtin_convertvector(rb, bf16x2_t);
    hi = make_uint2(H0.u, H1.u); lo = make_uint2(L0.u, L1.u);
}

// WW: GroupNorm groups of the layers the geometry flavours are made for (the dim-32 plan's; with the key's cpg: Cin = 4 cpg -- the launch
// path checks it), and window elements a thread of the run-time-geometry form may hold
constexpr int kFinGeomGroups = 4, kWWSlots = 8;

template <int WM, int WN, int WK, int MT, int NT, int CC, int NPL, int KS, int NL, int FL = FL_ALL, int PREC = 0, int GEOF = 0, int GEOK1 = 0>
__global__ void __launch_bounds__(256 + 64 * NL) conv_pipe_kernel(const ConvDev p_kernarg) {
    // the geometry key: GEOF on a Block-closing flavour, GEOK1 on a conv1 flavour (two template arguments, so that the route record and
    // the symbol names say which kind of key a launch carries); below it is one key, and FL_FIN tells the kinds apart
    static_assert(!(GEOF && GEOK1) && (!GEOF || (FL & FL_FIN)) && (!GEOK1 || !(FL & FL_FIN)), "one key per flavour, of its own kind");
    constexpr int GEO = GEOF != 0 ? GEOF : GEOK1;
    ConvDev p;
    conv_params_from_lanes(p);       // p_kernarg itself is never touched: see conv_dev.h
    constexpr int NTHR = 256 + 64 * NL, LT = 64 * NL;
    constexpr int BN = 32 * NT * WN, KSTEPS = CC / 2, KPW = KSTEPS / WK, Q = CC / 4, PIXSTEP = LT / Q, KK = KS * KS;
    static_assert(WM * WN * WK == 4, "4 consumer waves per workgroup");
    // DB ("direct B"): with one 32 x 32 output tile per workgroup every weight element feeds exactly one wave, so staging the slab in
    // LDS buys no reuse -- it only makes the loaders the pacemaker (stamps at 256->256 @4x4: loaders busy 37 k of the 43 k main-loop
    // cycles, consumers 43 % of theirs at the chunk barrier).  The consumers then load their K-quarter of the slab from global
    // straight into the MFMA B register layout (two 128-byte row segments per wave load), one chunk ahead, and the loaders keep
    // only the input window.
    constexpr bool DB = (WM * WN == 1 && MT == 1 && NT == 1 && KS == 3);
    // DB4 (round 3): the same with the weights in the k-step-quad layout (PACK_CONV_K8): a lane's B operands of the four k-steps its wave
    // owns in a chunk are ONE 16-byte load per tap (nine loads per chunk instead of 36, uniform base + 32-bit lane offset), and the two
    // register sets swap roles from chunk to chunk instead of being copied.  The copy was the round-2 kernel's hidden stall: the compiler
    // moved `wcur = wnxt` up to the last use of each wcur register, and every such move waits for a load issued moments earlier --
    // s_waitcnt vmcnt(35) in front of the chunk's FIRST MFMA, vmcnt(8) in front of its fourth: the "prefetch" was waited for at once
    // (ISA of <1,1,4,1,1,32,4,3,8,64>; 115 cycles per MFMA instead of 64).
    constexpr bool DB4 = DB && (FL & FL_W4) != 0;
#ifndef FC_DB4_CHAINS
#define FC_DB4_CHAINS 2
#endif
    constexpr int DB4_CHAINS = FC_DB4_CHAINS;
    // WW ("whole window", Block-closing DB4 flavours): the staging waves' GroupNorm / FiLM / SiLU work does not overlap the MFMAs of the
    // accumulator wave they share a SIMD with, and at 4x4 / 8x8 every column tile of a sample pair transforms the same
    // window.  Here ALL twelve waves stage every Cin chunk of the window, transformed, before the first MFMA -- the accumulator waves had
    // nothing to do until then -- at chunk i's place patch0 + i * patch_stride, in the per-chunk layout.  The K loop then holds no staging
    // and no chunk barrier; the staging waves wait at the barrier in front of the tail.  The launch path sizes the LDS (ww_lds below).
    constexpr bool WW = (FL & FL_WW) != 0;
    static_assert(!WW || (DB4 && FL != FL_ALL && (FL & FL_FIN) && (FL & FL_XF) && !(FL & (FL_CAT | FL_RES))), "whole-window staging: register-fed Block-closing flavours");
    // Pixel stride of the staged window in LDS.  CC + 1 keeps the dword operand reads of the MFMA lanes (one pixel per lane) off each other's
    // banks.  DB4 reads a lane's four k-steps of a tap as ONE 16-byte LDS read instead: inside every 8-channel block the window is stored
    // as [parity][4] (channel c at 8 (c / 8) + 4 (c & 1) + ((c >> 1) & 3)), so the channels 8 wk + 2 kk + half, kk = 0..3, are contiguous, and
    // the stride is a multiple of four floats (CC + 4) for the alignment the wide read needs.
    constexpr bool BF3 = PREC == 1;
    static_assert(!BF3 || (!DB && CC == 16 && FL == FL_ALL), "split-bf16: LDS-fed tiles, one 16-channel k-step per chunk, the all-in-one flavour");
    // BF3: the staging waves split the window on its way into LDS (a pixel is read by up to nine taps: splitting it at every read was half of
    // the accumulator waves' vector work): a pixel's 16 channels are stored as 16 bf16 hi parts | 16 bf16 lo parts (64 bytes) at the fp32
    // form's pitch of CC + 4 floats, so a lane's eight channels of either part are one 16-byte read.
    constexpr int CS = (DB4 || BF3) ? CC + 4 : CC + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ConvArgs& a = p.a;
    float* gstat = smem + p.o_gstat;
    float2* aff = reinterpret_cast<float2*>(smem + p.o_aff);   // [TB][Cin]
    float* patch0 = smem + p.o_patch;
    float* wl0 = smem + p.o_wl;
    const unsigned smem_lds = (unsigned)(size_t)(lptr_t)smem;      // LDS byte address of the dynamic segment

    const int tid = threadIdx.x, lane = tid & 63, wave8 = tid >> 6;
    const bool consumer = wave8 < 4;
    const int wave = wave8 & 3;                                   // consumer wave 0..3 (meaningless in a loader wave)
    const int lw = (wave8 - 4) & (NL - 1), ltid = (tid - 256) & (LT - 1);   // loader wave / loader thread (meaningless in a consumer wave)
    const int half = lane >> 5, l31 = lane & 31;
    const int wk = wave % WK, wn = (wave / WK) % WN, wm = wave / (WK * WN);

    // GEO1: the key on a conv1 flavour (conv_dev.h).  Such a layer has the dim-32 plan's kFinGeomGroups GroupNorm groups of cpg channels, a
    // 3x3 stride-1 window without upsampling or parity form -- conv1_geo_key() below tests all of it -- so the column tiles of the grid and
    // the window's extent are constants too: the tile decode and the staging threads' pixel decode divide by constants
    constexpr bool GEOC = GEO != 0, GEO1 = GEOC && !(FL & FL_FIN);
    constexpr int G1_NT = GEO1 ? geo_cpg(GEO) * kFinGeomGroups / BN : 1;
    static_assert(!GEO1 || (KS == 3 && geo_conv1_mask(FL) && geo_cpg(GEO) * kFinGeomGroups % BN == 0), "conv1 geometry flavours: 3x3, whole column tiles");
    const int bid = GEO1 ? xcd_remap(blockIdx.x, p.nblocks) : conv_parity_select(p, xcd_remap(blockIdx.x, p.nblocks));
    // tile decode without integer division: tiles_x / tiles_y are powers of two, ntiles goes through a host-made reciprocal
    const int mt_i = GEO1 ? bid / G1_NT : (p.ntiles == 1 ? bid : (p.magic_nt ? (int)__umulhi((unsigned)bid, p.magic_nt) : bid / p.ntiles));
    const int nt_i = bid - mt_i * (GEO1 ? G1_NT : p.ntiles);
    const int tx = mt_i & (p.tiles_x - 1), ty = (mt_i >> p.txl) & (p.tiles_y - 1), bg = mt_i >> (p.txl + p.tyl);
    // the tile geometry of a Block-closing flavour is a constant of the instantiation (GEO, conv_dev.h); a launch reaches it only when
    // every condition of fin_geo_key() below holds: one source without concat whose GroupNorm groups and statistics slots are those of
    // the output (Cin = Cout, same cpg, T = Tst), whole column tiles, tables of at most one entry per staging thread
    constexpr int BM = 32 * MT * WM;
    static_assert(!GEOC || GEO1 || (!(FL & FL_CAT) && (FL & FL_XF) && geo_Tst(GEO) <= kPartPre), "Block-closing geometry flavours: transform loader, one source");
    const int g_TB = GEOC ? geo_TB(GEO) : p.TB;
    const int g_TWl = GEOC ? geo_TWl(GEO) : p.TWl;
    const int g_tbsh = GEOC ? geo_log2(BM / geo_TB(GEO)) : p.TWl + p.THl;
    const int g_THl = GEOC ? geo_log2(BM / geo_TB(GEO)) - geo_TWl(GEO) : p.THl;
    const int TW = 1 << g_TWl, TH = 1 << g_THl;
    const int b0 = bg * g_TB, y0 = ty * TH, x0 = tx * TW, n0 = nt_i * BN;
    constexpr int G1_PW = GEO1 ? (1 << geo_TWl(GEO)) + 2 : 1, G1_PHW = GEO1 ? (BM / geo_TB(GEO) / (1 << geo_TWl(GEO)) + 2) * G1_PW : 1;
    const int PW = GEO1 ? G1_PW : p.PW, PHW = GEO1 ? G1_PHW : p.PH * p.PW;
    const int C0 = a.s0.C, C1 = a.s1.C, Cin = a.Cin, Cout = a.Cout;
    constexpr bool LEAN = FL != FL_ALL;        // launched for an exact match of the mask only: a set bit means "on"
    const bool has_res = LEAN ? bool(FL & FL_RES) : a.res_out != nullptr;
    const bool xf_on = LEAN ? bool(FL & FL_XF) : p.any_xf != 0;
    const int nchunks = p.nchunks;
    if (FL & FL_STAMP) conv_stamp(p, 0);
    // Fused tail across workgroups: draw this launch's epoch from the sample group's arrival counter NOW -- the round trip hides behind
    // the whole main loop; every workgroup of the group gets the same quotient because launches of one op never overlap.
    const bool meet = LEAN ? bool(FL & FL_MEET) : (a.fin.gamma != nullptr && !p.fin_local);
    // Inline asm on purpose: through the builtin, hipcc's atomic optimizer waits for the returned value on the spot (a cold round trip
    // in front of everything else); here the wait sits where the value is used, after the GroupNorm tables.
    unsigned arrival = 0;
    if (meet && tid == 0) {
        const gu32* cnt = (const gu32*)(a.fin.sync + b0 / g_TB);
        asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(arrival) : "v"(cnt), "v"(1u) : "memory");
    }
    // FL_STEP: with the epoch, the number of the evaluation this launch closes in its call (conv_dev.h "STEP") -- the sample's base epoch
    // and the call's number of evaluations are requested beside the arrival, so the tail finds the index in LDS
    // The block's header (pointers and constants of the call) is read here as well, into registers that live across the K loop: in the tail
    // it would be a cold round trip in front of every load the step needs.
    unsigned step_base = 0, step_n = 0;
    StepCloseHdr step_h;
    if constexpr ((FL & FL_STEP) != 0) {
        step_h = a.fin.step->h;
        step_n = (unsigned)step_h.n_slices;
        if (tid == 0) step_base = as_global(a.fin.step->base)[b0];
    }

    // ---- GroupNorm tables: moments per (sample, group), then the folded affine per (sample, channel).  The staging waves build them
    // AFTER they have put the first weight slabs in flight (two dependent global round trips that the slab transfer overlaps).
    // The tables are built by the staging waves alone (`worker`, thread `id` of `nthr`): the accumulator waves never read them, and a
    // second inlined copy of this code in their path was a few KB of cold instruction fetches per launch.  Both roles meet in the two barriers.
    auto gn_tables = [&](const bool worker, const int id, const int nthr) {
      if (xf_on) {
        const int G0 = a.s0.xf.mode ? a.s0.xf.G : 0, G1 = ((FL & FL_CAT) && a.s1.xf.mode) ? a.s1.xf.G : 0;
        // second-phase operands (gamma, beta, FiLM scale / shift of this thread's first (sample, channel) entry) are requested
        // together with the statistics: one memory round trip for the two tables instead of two dependent ones
        float pg = 1.f, pbt = 0.f, psc = 0.f, psh = 0.f;
        bool p_on = false, p_ss = false;
        int p_gs = 0;
       if (worker) {
        if (id < g_TB * Cin) {
            const int tb = GEOC ? ((geo_TB(GEO) > 1 && id >= Cin) ? 1 : 0) : id / Cin, c = id - tb * Cin, b = b0 + tb;
            const bool first = !(FL & FL_CAT) || c < C0;
            const SrcXform& xf = first ? a.s0.xf : a.s1.xf;
            if (b < a.B && xf.mode) {
                const int cs = first ? c : c - C0, Cs = first ? C0 : C1;
                p_on = true;
                p_gs = 2 * ((first ? 0 : p.TB * G0) + tb * xf.G + (GEOC ? cs / geo_cpg(GEO) : cs / (Cs / xf.G)));
                pg = xf.gamma[cs];
                pbt = xf.beta[cs];
                if (xf.ss) {
                    p_ss = true;
                    psc = xf.ss[(size_t)b * xf.ss_stride + cs];
                    psh = xf.ss[(size_t)b * xf.ss_stride + Cs + cs];
                }
            }
        }
        for (int i = id; i < g_TB * (G0 + G1); i += nthr) {
            const bool first = !(FL & FL_CAT) || i < p.TB * G0;
            const SrcXform& xf = first ? a.s0.xf : a.s1.xf;
            const int j = first ? i : i - p.TB * G0;
            const int tb = GEOC ? ((geo_TB(GEO) > 1 && j >= xf.G) ? 1 : 0) : j / xf.G, g = j - tb * xf.G, b = b0 + tb;
            float mean = 0.f, rstd = 0.f;
            if (b < a.B) {           // all partial pairs requested at once (stats_dev.h)
                if constexpr (GEOC) combine_partials_fixed<geo_Tst(GEO)>(xf, b, g, &mean, &rstd);
                else combine_partials(xf, b, g, &mean, &rstd);
            }
            gstat[2 * i] = mean;
            gstat[2 * i + 1] = rstd;
            if (GEOC) break;         // at most one (sample, group) per staging thread
        }
       }
        if ((FL & FL_STAMP) && worker) conv_stamp(p, 2);      // (staging rows) statistics combined: the first cold round trip is over
        // LDS-only barriers (round 4): the two tables are LDS data, and __syncthreads() also parks every wave until ALL its global
        // accesses have returned -- the accumulator waves' epoch atomic, epilogue operands and first weights, a second cold round trip
        // queued behind the statistics' one (tools/fin_stamps.py: statistics combined at 2.15 us, past this barrier at 3.12).  What a wave
        // needs from memory it waits for where it uses it; the staging waves' LDS-DMA has its own explicit wait before the hand-over.
        lds_only_barrier();
        if ((FL & FL_STAMP) && worker) conv_stamp(p, 4);
       if (worker) {
        if (id < g_TB * Cin) {
            float A = 1.f, Bv = 0.f;
            if (p_on) {
                A = gstat[p_gs + 1] * pg;
                Bv = pbt - gstat[p_gs] * A;
                if (p_ss) {
                    const float sc = psc + 1.0f;
                    A *= sc;
                    Bv = Bv * sc + psh;
                }
            }
            aff[id] = make_float2(A, Bv);
        }
        if (!GEOC)                   // (a geometry flavour: TB Cin <= staging threads)
        for (int i = id + nthr; i < p.TB * Cin; i += nthr) {
            const int tb = i / Cin, c = i - tb * Cin, b = b0 + tb;
            float A = 1.f, Bv = 0.f;
            const bool first = !(FL & FL_CAT) || c < C0;
            const SrcXform& xf = first ? a.s0.xf : a.s1.xf;
            if (b < a.B && xf.mode) {
                const int cs = first ? c : c - C0, Cs = first ? C0 : C1;
                const float* gs = gstat + 2 * ((first ? 0 : p.TB * G0) + tb * xf.G + cs / (Cs / xf.G));
                A = gs[1] * xf.gamma[cs];
                Bv = xf.beta[cs] - gs[0] * A;
                if (xf.ss) {
                    const float sc = xf.ss[(size_t)b * xf.ss_stride + cs] + 1.0f;
                    A *= sc;
                    Bv = Bv * sc + xf.ss[(size_t)b * xf.ss_stride + Cs + cs];
                }
            }
            aff[i] = make_float2(A, Bv);
        }
       }
        lds_only_barrier();
        if ((FL & FL_STAMP) && worker) conv_stamp(p, 5);      // (staging rows) the folded affine tables are in LDS
      }
    };

    f32x16 acc[MT][NT], accr[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[mt][nt][r] = 0.f; accr[mt][nt][r] = 0.f; }

    float pre[4 * NT];   // epilogue operands of this lane's columns (conv_dev.h): requested now, used after the last chunk
#pragma unroll
    for (int i = 0; i < 4 * NT; ++i) pre[i] = 0.f;
    if (consumer) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = n0 + (wn * NT + nt) * 32 + l31;
            if (n < Cout) {
                if (a.bias) pre[nt] = a.bias[n];
                if (has_res && a.res_b) pre[NT + nt] = a.res_b[n];
                if (a.fin.gamma) { pre[2 * NT + nt] = a.fin.gamma[n]; pre[3 * NT + nt] = a.fin.beta[n]; }
            }
        }
    }

    // ---- WW: this thread's share of the whole window.  Element e = tid + k NTHR is channel quad e % (Cin / 4) of window pixel e / (Cin / 4):
    // a pixel's channels are read by consecutive lanes.  A geometry flavour knows every count (kFinGeomGroups GroupNorm groups of cpg
    // channels, a TH x TW tile with its one-pixel halo) and unrolls fully; the run-time form keeps up to kWWSlots elements per thread.
    constexpr int WW_CQ = GEOC ? geo_cpg(GEO) * kFinGeomGroups / 4 : 0, WW_PW = GEOC ? (1 << geo_TWl(GEO)) + 2 : 0;
    constexpr int WW_PHW = GEOC ? (BM / geo_TB(GEO) / (1 << geo_TWl(GEO)) + 2) * WW_PW : 0, WW_E = GEOC ? geo_TB(GEO) * WW_PHW * WW_CQ : 0;
    constexpr int WWK = !WW ? 1 : (GEOC ? (WW_E + NTHR - 1) / NTHR : kWWSlots);
    f32x4 wv[WWK];
    int w_lds[WWK], w_aff[WWK];    // LDS float offset (-1: no element) / index of the affine pair (-1: padding or a sample beyond B: stays zero)
    const int ww_cq = GEOC ? WW_CQ : Cin >> 2, ww_pw = GEOC ? WW_PW : PW, ww_phw = GEOC ? WW_PHW : PHW, ww_E = GEOC ? WW_E : p.P * (Cin >> 2);
    const int ww_nk = GEOC ? WWK : __builtin_amdgcn_readfirstlane((ww_E + NTHR - 1) / NTHR);
    auto ww_request = [&]() {      // every load issued back to back; ordinary loads: they stay pending across gn_tables()
        const int Hin = a.Hs << a.ups, Win = a.Ws << a.ups;
        const float rcq = __builtin_amdgcn_rcpf((float)ww_cq);   // run-time form: e / ww_cq for e < 2^13 (ww_lds), exact with the half added
#pragma unroll
        for (int k = 0; k < WWK; ++k) {
            if (!GEOC && k >= ww_nk) break;
            const int e = tid + k * NTHR;
            w_lds[k] = -1; w_aff[k] = -1;
            const float* src = p.zeros16;
            if (e < ww_E) {
                const int pix = GEOC ? e / ww_cq : (int)(((float)e + 0.5f) * rcq), cq = e - pix * ww_cq;
                const int tb = GEOC ? pix / ww_phw : fastdiv(pix, p.magic_phw), r = pix - tb * ww_phw;
                const int py = GEOC ? r / ww_pw : fastdiv(r, p.magic_pw), px = r - py * ww_pw;
                const int iy = y0 * a.stride - (a.pad_y >= 0 ? a.pad_y : a.pad) + py, ix = x0 * a.stride - (a.pad_x >= 0 ? a.pad_x : a.pad) + px, b = b0 + tb;
                if (b < a.B && iy >= 0 && iy < Hin && ix >= 0 && ix < Win) {
                    src = a.s0.p + (size_t)((b * a.Hs + (iy >> a.ups)) * a.Ws + (ix >> a.ups)) * C0 + 4 * cq;
                    w_aff[k] = tb * Cin + 4 * cq;
                }
                w_lds[k] = (cq >> 3) * p.patch_stride + pix * CS + 8 * ((cq & 7) >> 1) + 2 * (cq & 1);
            }
            wv[k] = *reinterpret_cast<const f32x4*>(src);
        }
    };
    auto ww_store = [&]() {        // ... and on into LDS, transformed exactly as the per-chunk loader's store_patch does
#pragma unroll
        for (int k = 0; k < WWK; ++k) {
            if (!GEOC && k >= ww_nk) break;
            if (w_lds[k] < 0) continue;
            f32x4 x = wv[k];
            if (w_aff[k] >= 0) {
                const float2* ab = aff + w_aff[k];
                x.x = ab[0].x * x.x + ab[0].y; x.y = ab[1].x * x.y + ab[1].y;
                x.z = ab[2].x * x.z + ab[2].y; x.w = ab[3].x * x.w + ab[3].y;
                if (p.act0) { x.x = silu_f(x.x); x.y = silu_f(x.y); x.z = silu_f(x.z); x.w = silu_f(x.w); }
            }
            float* d = patch0 + w_lds[k];
            d[0] = x.x; d[1] = x.z; d[4] = x.y; d[5] = x.w;      // [parity][4] inside the 8-channel block
        }
    };

    if (!consumer) {
        // =========================================== LOADERS ===========================================
      if constexpr (WW) {
        ww_request();
        if (FL & FL_STAMP) conv_stamp(p, 1);
        gn_tables(true, ltid, LT);
        ww_store();
        if (FL & FL_STAMP) conv_stamp(p, 3);      // (staging rows) the whole window is in LDS
        loader_handover();                        // every chunk ready; nothing left to stage: on to the barrier in front of the tail
      } else {
        // Waves 4+ are the younger half of the workgroup: at equal priority the SIMD's issue arbitration (priority, then age) hands them
        // the slots the MFMA waves leave over, and the consumers then sit at the chunk barrier waiting for a stage the loaders could
        // not issue fast enough (stamps: 5 k cycles to issue three loads per thread).  s_setprio is scalar: the branch is wave-uniform.
        {
            const int lp = __builtin_amdgcn_readfirstlane(p.loader_prio);
            if (lp == 1) __builtin_amdgcn_s_setprio(1);
            else if (lp == 2) __builtin_amdgcn_s_setprio(2);
            else if (lp == 3) __builtin_amdgcn_s_setprio(3);
        }
        const float* wbase = a.w + (size_t)b0 * a.w_batch_stride;
        const int q4 = (ltid % Q) * 4;
        int e_po[NPL], e_lds[NPL], e_tb[NPL];   // this thread's patch elements: pixel (ltid/Q + k*256/Q), channel quad ltid%Q
        {
            const int Hin = a.Hs << a.ups, Win = a.Ws << a.ups;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const int pix = ltid / Q + k * PIXSTEP;
                e_po[k] = -1; e_lds[k] = -1; e_tb[k] = 0;
                if (GEO1) {           // the window's extent is a constant of the key: divisions by constants, stride 1, pad 1, no upsampling
                    if (pix < geo_TB(GEO) * G1_PHW) {
                        const int tb = pix / G1_PHW, r = pix - tb * G1_PHW, py = r / G1_PW, px = r - py * G1_PW;
                        const int iy = y0 - 1 + py, ix = x0 - 1 + px, b = b0 + tb;
                        if (b < a.B && iy >= 0 && iy < a.Hs && ix >= 0 && ix < a.Ws) e_po[k] = (b * a.Hs + iy) * a.Ws + ix;
                        e_lds[k] = pix * CS + (DB4 ? 8 * ((ltid % Q) >> 1) + 2 * ((ltid % Q) & 1) : q4);
                        e_tb[k] = tb;
                    }
                } else if (pix < p.P) {
                    const int tb = fastdiv(pix, p.magic_phw), r = pix - tb * PHW, py = fastdiv(r, p.magic_pw), px = r - py * PW;
                    const int iy = y0 * a.stride - (a.pad_y >= 0 ? a.pad_y : a.pad) + py, ix = x0 * a.stride - (a.pad_x >= 0 ? a.pad_x : a.pad) + px, b = b0 + tb;
                    if (b < a.B && iy >= 0 && iy < Hin && ix >= 0 && ix < Win) e_po[k] = (b * a.Hs + (iy >> a.ups)) * a.Ws + (ix >> a.ups);
                    e_lds[k] = pix * CS + (DB4 ? 8 * ((ltid % Q) >> 1) + 2 * ((ltid % Q) & 1) : q4);
                    e_tb[k] = tb;
                }
            }
        }
        if (FL & FL_STAMP) conv_stamp(p, 1);
        const int nwb = p.nwb;                    // weight stages in LDS: 3 = slabs run two chunks ahead, 2 = one ahead
        // LDS-DMA plan of this lw: piece j = lw + 4m covers 256 floats of the slab = (256/BN) rows x BN columns.  A lane's
        // source pointer at chunk 0 is fixed for the whole kernel and advances by CC*Cout floats per chunk, so issuing a slab
        // costs one 64-bit add + one scalar add per piece (the address arithmetic used to outweigh the transfer: the loaders,
        // not the MFMA waves, set the pace of the small-M layers -- profiles/r01_c_stamps.txt).
        constexpr int MAXP = ((KK + 1) * CC * BN / 256 + NL - 1) / NL;
        const int rows_main = KK * CC, npieces = (rows_main + (has_res ? CC : 0)) * BN / 256;
        const int my_pieces = __builtin_amdgcn_readfirstlane(npieces > lw ? (npieces - lw + NL - 1) / NL : 0);
        const float* d_ptr[MAXP];   // nullptr: column beyond Cout -> zero block
        int d_row[MAXP];            // channel row inside the chunk (for the Cin tail test)
#pragma unroll
        for (int m = 0; m < MAXP; ++m) {
            const int j = lw + NL * m, f = j * 256 + lane * 4, row = f / BN, n = n0 + (f % BN);
            if constexpr (BF3) {
                // split-bf16 slab [part hi/lo][tap][channel block of 8 (two per chunk)][BN] x 16 bytes, read from the pre-split copy of the
                // weights (PACK_CONV_B3: per part [tap][Ipad/8][Cout] x 16 bytes, Ipad = 16 nchunks, zero beyond Cin): one lane, one column's
                // eight channels.  Same byte count per chunk as the fp32 slab, so the piece bookkeeping is shared
                const int e = j * 64 + lane, r = e / BN, nn = n0 + e % BN, part = r / (2 * KK), tap = (r >> 1) % KK, c8l = r & 1;
                d_row[m] = 0;
                d_ptr[m] = (nn >= Cout || part > 1) ? nullptr
                         : a.w_b3 + (size_t)part * ((size_t)KK * nchunks * 8 * Cout) + ((size_t)(tap * 2 * nchunks + c8l) * Cout + nn) * 4;
                continue;
            }
            const bool res = row >= rows_main;
            d_row[m] = res ? row - rows_main : row % CC;
            d_ptr[m] = n >= Cout ? nullptr : (res ? a.res_w + (size_t)d_row[m] * Cout + n : wbase + ((size_t)(row / CC) * Cin + d_row[m]) * Cout + n);
        }
        auto dma_weights = [&](int i) {
            const int c0 = i * CC;
            const size_t adv = BF3 ? (size_t)i * 8 * Cout : (size_t)c0 * Cout;
            const unsigned wb = smem_lds + 4u * (unsigned)(p.o_wl + (i % nwb) * p.wl_stride + lw * 256);
            const bool tail = !BF3 && c0 + CC > Cin;    // only the last chunk can run past Cin (the split-bf16 copy is padded with zeros)
#pragma unroll
            for (int m = 0; m < MAXP; ++m) {
                if (m >= my_pieces) break;
                const bool ok = d_ptr[m] != nullptr && (!tail || c0 + d_row[m] < Cin);
                lds_dma16(ok ? d_ptr[m] + adv : p.zeros16, wb + 4u * (unsigned)(m * (NL * 256)));
            }
        };
        f32x4 pv[NPL];
        const int nk = GEO1 ? (geo_TB(GEO) * G1_PHW * Q + LT - 1) / LT : __builtin_amdgcn_readfirstlane((p.P * Q + LT - 1) / LT);   // element slots in use (scalar: cheap loop exits)
        auto issue_patch = [&](int i, f32x4 (&pv)[NPL]) {   // input window of chunk i -> registers, every load issued back to back
            const int c = i * CC + q4;
            const bool live = c < Cin, first = !(FL & FL_CAT) || c < C0;
            const float* base = first ? a.s0.p + c : a.s1.p + (c - C0);
            const int Cs = first ? C0 : C1;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {       // padding / out-of-range elements read the zero block: no branches, zeros arrive
                if (k >= nk) break;
                hidden_load16(pv[k], (live && e_po[k] >= 0) ? base + (size_t)e_po[k] * Cs : p.zeros16);
            }
        };
        auto store_patch = [&](int i, f32x4 (&pv)[NPL]) {   // ... and on into LDS with GroupNorm / FiLM / SiLU applied
            const int c = i * CC + q4;
            float* pb = patch0 + (i & 1) * p.patch_stride;
            const bool live = c < Cin, act = (c < C0) ? p.act0 : p.act1;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                if (k >= nk) break;
                if (e_lds[k] < 0) continue;
                f32x4 x = pv[k];
                if (xf_on && live && e_po[k] >= 0) {
                    const float2* ab = aff + e_tb[k] * Cin + c;
                    x.x = ab[0].x * x.x + ab[0].y; x.y = ab[1].x * x.y + ab[1].y;
                    x.z = ab[2].x * x.z + ab[2].y; x.w = ab[3].x * x.w + ab[3].y;
                    if (act) { x.x = silu_f(x.x); x.y = silu_f(x.y); x.z = silu_f(x.z); x.w = silu_f(x.w); }
                }
                float* d = pb + e_lds[k];
                if (BF3) {                                                        // hi parts at byte 2 c, lo parts at byte 2 CC + 2 c of the pixel
                    uint2 h2, l2;
                    split_bf16x4(x, h2, l2);
                    char* pc = reinterpret_cast<char*>(pb + (e_lds[k] - q4)) + 2 * q4;
                    *reinterpret_cast<uint2*>(pc) = h2;
                    *reinterpret_cast<uint2*>(pc + 2 * CC) = l2;
                }
                else if (DB4) { d[0] = x.x; d[1] = x.z; d[4] = x.y; d[5] = x.w; }      // [parity][4] inside the 8-channel block
                else { d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w; }
            }
        };
        unsigned long long dbg_mem = 0, dbg_store = 0, dbg_bar = 0, dbg_issue = 0, dbg_dma = 0;   // diagnostics: cycles per loader phase
        if (!DB) {
            dma_weights(0);
            if (nwb == 3 && nchunks > 1) dma_weights(1);
        }
        {   // window 0 does not depend on the tables: request it first, so that its round trip overlaps theirs.  Ordinary loads --
            // the compiler must see them pending across gn_tables() (hidden loads are only safe in straight-line code).
            const int c = q4;
            const bool live = c < Cin, first = !(FL & FL_CAT) || c < C0;
            const float* base = first ? a.s0.p + c : a.s1.p + (c - C0);
            const int Cs = first ? C0 : C1;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                if (k >= nk) break;
                pv[k] = *reinterpret_cast<const f32x4*>((live && e_po[k] >= 0) ? base + (size_t)e_po[k] * Cs : p.zeros16);
            }
        }
        gn_tables(true, ltid, LT);
        store_patch(0, pv);
        if (FL & FL_STAMP) conv_stamp(p, 3);
        // EXPLICIT, unconditional wait for this wave's slab pieces before stage 0 is handed over (round 4; the root cause of the results
        // that differed when two replicas ran side by side).  The LDS-DMA above is invisible to the compiler, so until now the only thing
        // that retired it was the compiler's own wait for the window loads in store_patch -- and that wait sits INSIDE the `e_lds >= 0`
        // branch: a loader wave none of whose lanes has a window element (the folded-upsampling launch at 4x4: 2 samples x 5 x 5 window
        // pixels x 8 channel quads = 400 elements for 512 loader threads, wave 7 idle) skipped it (s_cbranch_execz) and reached the barrier
        // with its pieces -- rows 56..63 of taps 1 and 3 -- possibly still in flight; the consumers then multiplied whatever the previous
        // workgroup had left in that LDS.  Alone on the GPU the pieces, requested a memory round trip before the window, had always landed;
        // beside a second stream's kernels they sometimes had not (tools/race_hunt.py: first differing tensor ups.0.3, one parity class, one
        // 32-column tile, exactly the pixels tap 1 or tap 3 reaches).  Busy waves drained to zero here already (the compiler's wait counts
        // only its own, younger loads), so this costs nothing.  Issued as the BUILTIN (a real S_WAITCNT instruction, vmcnt(0) with the other
        // counters left alone), not as inline asm: the compiler's wait-count pass reads it and then KNOWS that the window loads above have
        // completed on every path.  Without that knowledge it assumed they might still be pending wherever a lane had skipped its store, and
        // protected the registers they share with the hidden loads of the loop by an `s_waitcnt vmcnt(0)` in front of the loop's window
        // requests and another in front of every LDS store -- each of which also drained the slab that was meant to stay in flight.
        __builtin_amdgcn_s_waitcnt(0x0F70);
        loader_handover();                        // stage 0 ready
        for (int g = 0; g < nchunks; ++g) {       // consumers are on chunk g
            const bool next = g + 1 < nchunks;
            int ahead = 0;
            unsigned long long ta = ((FL & FL_STAMP) && p.stamps) ? __builtin_amdgcn_s_memtime() : 0ull;
            if (!DB && next && nwb == 2) dma_weights(g + 1);
            if (next) issue_patch(g + 1, pv);
            unsigned long long tb_ = ((FL & FL_STAMP) && p.stamps) ? __builtin_amdgcn_s_memtime() : 0ull;
            if (!DB && nwb == 3 && g + 2 < nchunks) { dma_weights(g + 2); ahead = my_pieces; }
            unsigned long long t0 = ((FL & FL_STAMP) && p.stamps) ? __builtin_amdgcn_s_memtime() : 0ull;
            if ((FL & FL_STAMP) && p.stamps) { dbg_issue += tb_ - ta; dbg_dma += t0 - tb_; }
            wait_vmcnt(ahead);                    // window g+1 in registers, slab g+1 landed; slab g+2 stays in flight across the barrier
            unsigned long long t1 = ((FL & FL_STAMP) && p.stamps) ? __builtin_amdgcn_s_memtime() : 0ull;
            if (next) store_patch(g + 1, pv);
            unsigned long long t2 = ((FL & FL_STAMP) && p.stamps) ? __builtin_amdgcn_s_memtime() : 0ull;
            loader_handover();
            if ((FL & FL_STAMP) && p.stamps) { dbg_mem += t1 - t0; dbg_store += t2 - t1; dbg_bar += __builtin_amdgcn_s_memtime() - t2; }
        }
        if ((FL & FL_STAMP) && p.stamps && lane == 0) {
            unsigned long long* d = p.stamps + ((size_t)blockIdx.x * 8 + (wave8 < 8 ? wave8 : 7)) * 16;
            d[9] = dbg_mem; d[10] = dbg_store; d[11] = dbg_bar; d[12] = dbg_issue; d[13] = dbg_dma;
        }
        __builtin_amdgcn_s_setprio(0);   // staging is over: in the epilogue the accumulator waves are the ones with work to do
      }
    } else {
        // =========================================== CONSUMERS ===========================================
        int abase[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = (wm * MT + mt) * 32 + l31;
            const int tw = m & (TW - 1), th = (m >> g_TWl) & (TH - 1), tb = m >> g_tbsh;
            const int st = GEO1 ? 1 : a.stride;
            abase[mt] = (tb * PHW + th * st * PW + tw * st) * CS + half;
        }
        const int bbase = half * BN + wn * NT * 32 + l31;
        const int kk0 = wk * KPW;
        const int abase4 = abase[0] - half + 8 * wk + 4 * half;     // DB4: this lane's [parity][4] quad of its wave's 8-channel block
        unsigned long long dbg_cbar = 0;
        constexpr int NB = (DB && !DB4) ? KK * KPW : 1, NR = (DB && !DB4) ? KPW : 1;
        float wcur[NB], wnxt[NB], rcur[NR], rnxt[NR];
        const int ncol = n0 + l31;
        const bool colok = ncol < Cout;                 // a column beyond Cout reads the zero block with zero strides
        const float* wq = colok ? a.w + (size_t)b0 * a.w_batch_stride + ncol : p.zeros16;
        const float* rq = (colok && has_res) ? a.res_w + ncol : p.zeros16;
        const size_t wcs = colok ? (size_t)Cout : 0, wts = colok ? (size_t)Cin * Cout : 0;
        auto fetch_w = [&](int i, float (&w)[NB], float (&r)[NR]) {   // this wave's rows of chunk i: channel c of every tap (+ res_conv row)
#pragma unroll
            for (int kk = 0; kk < KPW; ++kk) {
                int c = i * CC + 2 * (kk0 + kk) + half;
                c = c < Cin ? c : Cin - 1;               // past the Cin tail the window holds zeros: any finite weight will do
                const float* q = wq + (size_t)c * wcs;
#pragma unroll
                for (int tap = 0; tap < KK; ++tap) w[tap * KPW + kk] = q[(size_t)tap * wts];
                if (has_res) r[kk] = rq[(size_t)c * wcs];
            }
        };
        // DB4: registers A / B, each the nine taps' float4 (component j = k-step kk0 + j) of one chunk, plus the res_conv quad
        constexpr int NQ = DB4 ? KK : 1;
        f32x4 wA[NQ], wB[NQ], rA, rB;
        const unsigned lane_off4 = DB4 ? (unsigned)(half * Cout + ncol) * 4u : 0u;       // floats; DB4 launches have Cout % 32 == 0: every column exists
        const int wk_u = __builtin_amdgcn_readfirstlane(wk);
        auto fetch4 = [&](int i, f32x4 (&w)[NQ], f32x4& r) {
            // uniform base: chunk i, this wave's K-quarter = row block c8 = i * (CC / 8) + wk of [tap][Cin/8][half][Cout][4]
            const size_t blk = (size_t)((i * (CC / 8) + wk_u) * 2) * (size_t)Cout * 4;
            const float* ub = a.w4 + blk;
#pragma unroll
            for (int tap = 0; tap < NQ; ++tap) w[tap] = *reinterpret_cast<const f32x4*>(ub + (size_t)tap * ((size_t)Cin * Cout) + lane_off4);
            if (has_res) r = *reinterpret_cast<const f32x4*>(a.res_w4 + blk + lane_off4);
        };
        if (DB4) fetch4(0, wA, rA);
        else if (DB) fetch_w(0, wcur, rcur);
        if constexpr (WW) ww_request();
        if (FL & FL_STAMP) conv_stamp(p, 1);
        gn_tables(false, 0, 1);
        if constexpr (WW) ww_store();
        if (meet && tid == 0) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(arrival) :: "memory");
            smem[p.o_epoch] = __uint_as_float(arrival / (unsigned)p.gsz + 1u);
            if constexpr ((FL & FL_STEP) != 0) {     // the NEXT evaluation's number, never past the call's last; whether it has a conditioning slice
                const unsigned nxt = min(arrival / (unsigned)p.gsz + 1u - step_base + 1u, step_n);
                smem[p.o_epoch + 1] = __uint_as_float(nxt);
                smem[p.o_epoch + 2] = __uint_as_float(nxt < step_n ? 1u : 0u);
            }
        }
        __syncthreads();        // stage 0 ready
        if (FL & FL_STAMP) conv_stamp(p, 4);
        f32x16 acc2;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
        if constexpr (DB4) {
            // one chunk on register set `wc`, the next chunk's weights requested into `wn` first: they are not read before the NEXT chunk
            // (a whole chunk of MFMAs of lookahead), and nothing is copied.  The A operands of tap t + 1 are read from LDS before the
            // MFMAs of tap t are issued.
            auto chunk = [&](int i, f32x4 (&wc)[NQ], f32x4& rc, f32x4 (&wn)[NQ], f32x4& rn) {
                const float* patch = patch0 + (WW ? i : (i & 1)) * p.patch_stride;
                // UNCONDITIONAL (the last chunk re-requests itself): s_waitcnt takes an immediate, so with a conditional request the
                // compiler must count for the path that skipped it -- vmcnt(8) instead of vmcnt(17) in front of the first MFMA, i.e. a wait
                // for the request issued two lines above
                fetch4(i + 1 < nchunks ? i + 1 : i, wn, rn);
                __builtin_amdgcn_sched_barrier(0);       // the requests stay HERE: left alone, the scheduler sinks them behind the chunk's MFMAs
                static_assert(!DB4 || KPW == 4, "one 16-byte operand read = the four k-steps of a wave");
                (void)patch;
                // Pinned schedule: the operand quad of tap t + 1 is requested (asm: the compiler neither counts nor moves it), then the four
                // MFMAs of tap t run -- 256 cycles of cover for the LDS round trip --, then the wait.  Left to the scheduler the reads
                // ended up directly in front of their first use (s_waitcnt lgkmcnt right behind ds_read, every eighth MFMA).
                const unsigned pl = smem_lds + 4u * (unsigned)(p.o_patch + (WW ? i : (i & 1)) * p.patch_stride + abase4);
                const unsigned prow = 4u * (unsigned)(PW * CS);
                auto lds_quad = [&](f32x4& dst, int tapn) {
                    const unsigned ad = pl + (unsigned)(tapn / KS) * prow;
                    switch (tapn % KS) {         // column offset as an immediate
                        case 0: asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(ad) : "memory"); break;
                        case 1: asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(ad), "n"(4 * CS) : "memory"); break;
                        default: asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(ad), "n"(8 * CS) : "memory"); break;
                    }
                };
                f32x4 av, an;
                lds_quad(av, 0);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av) :: "memory");
                an = av;
#pragma unroll
                for (int tap = 0; tap < KK; ++tap) {
                    // (after the last tap: the centre tap again, for the fused res_conv)
                    if (tap + 1 < KK || has_res) lds_quad(an, tap + 1 < KK ? tap + 1 : KK / 2);
                    __builtin_amdgcn_sched_barrier(0);
                    if (DB4_CHAINS == 2) {
                        // two independent accumulator chains: an MFMA that waits for its predecessor's result seems to hold the SIMD's issue
                        // port while it waits, and the staging waves that share the SIMD starve (stamps, round 3)
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], wc[tap][0], acc[0][0], 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], wc[tap][1], acc2, 0, 0, 0);
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], wc[tap][2], acc[0][0], 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], wc[tap][3], acc2, 0, 0, 0);
                    } else {
#pragma unroll
                        for (int kk = 0; kk < KPW; ++kk) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], wc[tap][kk], acc[0][0], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (tap + 1 < KK || has_res) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(an) :: "memory");
                    av = an;
                }
                if (has_res) {
#pragma unroll
                    for (int kk = 0; kk < KPW; ++kk) accr[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], rc[kk], accr[0][0], 0, 0, 0);
                }
                if constexpr (!WW) {                     // (WW: every chunk is in LDS already, nothing is handed over)
                unsigned long long t0 = ((FL & FL_STAMP) && p.stamps) ? __builtin_amdgcn_s_memtime() : 0ull;
                loader_handover();                       // not __syncthreads(): its vmcnt(0) would wait for the weights requested above
                if ((FL & FL_STAMP) && p.stamps) dbg_cbar += __builtin_amdgcn_s_memtime() - t0;
                }
            };
            for (int i = 0; i < nchunks; i += 2) {
                chunk(i, wA, rA, wB, rB);
                if (i + 1 < nchunks) chunk(i + 1, wB, rB, wA, rA);
            }
            if (DB4_CHAINS == 2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][0][r] += acc2[r];
            }
        } else if constexpr (BF3) {
            // lane (row / column l31, half): channels 8 half .. 8 half + 7 of each 16-channel k-step, of its pixel (A) and of its column (B)
            int ab3[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) ab3[mt] = abase[mt] - half + 4 * half;    // (16 bytes per half: eight bf16)
            const int bb3 = 4 * (half * BN + wn * NT * 32 + l31);    // floats: 16 bytes per (channel block, column)
            static_assert(CC == 16, "one k-step of sixteen channels per tap");
            typedef union { uint4 u; bf16x8_t v; } opnd_t;
            for (int i = 0; i < nchunks; ++i) {
                const float* patch = patch0 + (i & 1) * p.patch_stride;
                const float* wl = wl0 + (i % p.nwb) * p.wl_stride + bb3;
                // (The scheduler is left alone here.  A pinned schedule -- operands of tap t + 1 requested, then the 3 MT NT MFMAs of tap t
                // back to back -- measured 376 images/s against 421 on the SD-VAE decode: the staging waves' VALU work does not overlap the
                // MFMAs of the wave that shares their SIMD, DESIGN.md section 5, and a dense MFMA stream only moves the waiting around.)
#pragma unroll
                for (int tap = 0; tap < KK; ++tap) {
                    const int tapoff = ((tap / KS) * PW + (tap % KS)) * CS;
                    opnd_t A[MT][2], Bq[NT][2];       // [tile][hi / lo]
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {  // split by the staging waves: 16 bytes of hi parts, 16 bytes of lo parts per pixel and half
                        const char* pc = reinterpret_cast<const char*>(patch + ab3[mt] + tapoff);
                        A[mt][0].u = *reinterpret_cast<const uint4*>(pc);
                        A[mt][1].u = *reinterpret_cast<const uint4*>(pc + 2 * CC);
                    }
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {  // split at pack time, staged by LDS-DMA
                        Bq[nt][0].u = *reinterpret_cast<const uint4*>(wl + 4 * ((tap * 2) * BN + nt * 32));
                        Bq[nt][1].u = *reinterpret_cast<const uint4*>(wl + 4 * (((KK + tap) * 2) * BN + nt * 32));
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][1].v, Bq[nt][0].v, acc[mt][nt], 0, 0, 0);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0].v, Bq[nt][1].v, acc[mt][nt], 0, 0, 0);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0].v, Bq[nt][0].v, acc[mt][nt], 0, 0, 0);
                        }
                }
                __syncthreads();    // stage i consumed; stage i + 1 (if any) ready
            }
        } else {
        for (int i = 0; i < nchunks; ++i) {
            const float* patch = patch0 + (i & 1) * p.patch_stride;
            const float* wl = wl0 + (i % p.nwb) * p.wl_stride + bbase;
            if (DB && i + 1 < nchunks) fetch_w(i + 1, wnxt, rnxt);
#pragma unroll
            for (int tap = 0; tap < KK; ++tap) {
                const int tapoff = ((tap / KS) * PW + (tap % KS)) * CS;
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk) {
                    const int k = 2 * (kk0 + kk);
                    float av[MT], bv[NT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) av[mt] = patch[abase[mt] + tapoff + k];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bv[nt] = DB ? wcur[tap * KPW + kk] : wl[(tap * CC + k) * BN + nt * 32];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
                }
            }
            if (has_res) {   // fused res_conv: the centre tap against its own weight slab
                const int tapoff = GEO1 ? (PW + 1) * CS : (a.pad * PW + a.pad) * CS;
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk) {
                    const int k = 2 * (kk0 + kk);
                    float av[MT], bv[NT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) av[mt] = patch[abase[mt] + tapoff + k];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bv[nt] = DB ? rcur[kk] : wl[(KK * CC + k) * BN + nt * 32];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            accr[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], accr[mt][nt], 0, 0, 0);
                }
            }
            unsigned long long t0 = ((FL & FL_STAMP) && p.stamps) ? __builtin_amdgcn_s_memtime() : 0ull;
            if (DB) {
                loader_handover();                       // not __syncthreads(): its vmcnt(0) would wait for the slab prefetched above
#pragma unroll
                for (int j = 0; j < NB; ++j) wcur[j] = wnxt[j];
#pragma unroll
                for (int j = 0; j < NR; ++j) rcur[j] = rnxt[j];
            } else {
                __syncthreads();    // stage i consumed; stage i+1 (if any) ready
            }
            if ((FL & FL_STAMP) && p.stamps) dbg_cbar += __builtin_amdgcn_s_memtime() - t0;
        }
        }
        if ((FL & FL_STAMP) && p.stamps && lane == 0) p.stamps[((size_t)blockIdx.x * 8 + wave8) * 16 + 11] = dbg_cbar;
        if (FL & FL_STAMP) conv_stamp(p, 5);
    }
    // WW: the one barrier the K loop no longer has -- every accumulator wave has read its last operands, the window (which the tail's
    // scratch aliases) is dead.  lgkmcnt only: a wave's outstanding global requests are not waited for here
    if constexpr (WW) loader_handover();
    conv_epilogue<WM, WN, WK, MT, NT, FL, GEO>(p, acc, accr, smem, tid, lane, wave, b0, y0, x0, n0, tx, ty, consumer, NTHR, pre, true, &step_h);
}

// ---------------------------------------------------------------------------------------------------
static float* g_zeros16 = nullptr;
const float* conv_zeros16() { return g_zeros16; }

// Every instantiation of conv_pipe_kernel is one row of a table built once, in conv_pipe_init(): what a launch is matched on -- tile,
// kernel size, flavour mask (conv_dev.h FL_*, the form bits FL_W4 / FL_WW / FL_STEP included), precision and the two geometry keys --
// and what it then runs.  conv_pipe_select() picks the row of a launch; the launch, the occupancy query, the route record and the LDS
// attribute are each written once, against the row.
struct PipeRow {
    int tile;
    int targ[13];                   // the template arguments: the instantiation's name in the code object's symbol table, and its route record
    void (*fn)(const ConvDev);
    int nthr;
    unsigned long long key;         // pipe_key() of the match fields
};
enum { A_NPL = 6, A_FL = 9 };       // positions in PipeRow::targ (WM WN WK MT NT CC NPL KS NL FL PREC GEOF GEOK1)
// The selection runs in front of every eager launch (a training step has some two hundred), so the table is sorted by key and indexed by
// (tile, kernel size), the key's leading bits: the rows of bucket b are g_begin[b] .. g_begin[b + 1], and g_keys holds their keys
// side by side, so that a search reads a few consecutive cache lines.  (Before conv_pipe_init() every bucket is empty.)
static std::vector<PipeRow> g_rows;
static std::vector<PipeRow>* g_fill = &g_rows;    // where build_rows() puts its rows: the table, or the listing of conv_table_list()
static std::vector<unsigned long long> g_keys;
constexpr int kBuckets = TILE_COUNT * 16;
static int g_begin[kBuckets + 1];

static unsigned long long pipe_key(int tile, int ks, int fl, int prec, int geof, int geok1) {     // add_row() asserts the field widths
    typedef unsigned long long u64;
    return (u64)(tile * 16 + ks) << 49 | (u64)prec << 48 | (u64)fl << 32 | (u64)geof << 16 | (u64)geok1;
}

// The one place that names an instantiation: everything about the tile comes from kConvTiles, the staging elements per thread from the
// mask (conv_dev.h kPipeNPL / kLeanNPL).  A split-bf16 row exists where conv_geometry() may set ConvDev::bf3, and nowhere else.
template <int TILE, int KS, int FL, int PREC = 0, int GEOF = 0, int GEOK1 = 0>
static void add_row() {
    static_assert(KS < 16 && PREC < 2 && FL < (1 << 16) && GEOF < (1 << 16) && GEOK1 < (1 << 16), "the fields of pipe_key()");
    if constexpr (PREC == 0 || conv_bf3_form(TILE, KS)) {
        constexpr ConvTileDef t = kConvTiles[TILE];
        constexpr int NPL = FL == FL_ALL ? kPipeNPL : kLeanNPL, NL = conv_tile_nl(TILE, KS);
        g_fill->push_back({TILE, {t.WM, t.WN, t.WK, t.MT, t.NT, t.CC, NPL, KS, NL, FL, PREC, GEOF, GEOK1},
                          &conv_pipe_kernel<t.WM, t.WN, t.WK, t.MT, t.NT, t.CC, NPL, KS, NL, FL, PREC, GEOF, GEOK1>, 256 + 64 * NL,
                          pipe_key(TILE, KS, FL, PREC, GEOF, GEOK1)});
    }
}
template <int KS, int FL, int PREC = 0, int... TILES>
static void add_tiles(std::integer_sequence<int, TILES...>) { (add_row<TILES, KS, FL, PREC>(), ...); }

// The all-in-one kernel (FL_ALL) exists for every tile; lean flavours for the tiles the U-Net runs on: 3x3 as plain / + fused res_conv /
// + fused tail, 1x1 and 2x2 plain.  Everything else goes to the all-in-one instantiation.
// (The order of the tiles in a list, like that of the rows, carries no meaning.)
using AllTiles = std::integer_sequence<int, TILE_M256N64, TILE_M64N64K2, TILE_M32N32K4, TILE_M64N32K2, TILE_M128N64, TILE_M128N32>;
using LeanTiles = std::integer_sequence<int, TILE_M32N32K4, TILE_M64N32K2, TILE_M128N32>;
// the 64-column tiles the 1x1 projections of the larger models run on (to_qkv and its data gradient): lean flavours for 1x1 only
using Wide1Tiles = std::integer_sequence<int, TILE_M256N64, TILE_M128N64>;

#define FC_LEAN_FLAVOURS_3(X) X(0) X(FL_POSTOP) X(FL_STATS) X(FL_STATS | FL_STAMP) X(FL_STATS | FL_CAT | FL_STAMP) X(FL_STATS | FL_RES) X(FL_STATS | FL_CAT) X(FL_STATS | FL_RES | FL_CAT) X(FL_STATS | FL_XF) \
    X(FL_STATS | FL_XF | FL_FIN) X(FL_STATS | FL_XF | FL_FIN | FL_GN1) X(FL_STATS | FL_XF | FL_FIN | FL_MEET) X(FL_STATS | FL_XF | FL_FIN | FL_GN1 | FL_MEET) \
    X(FL_STATS | FL_XF | FL_FIN | FL_STAMP) X(FL_STATS | FL_XF | FL_FIN | FL_GN1 | FL_STAMP) X(FL_STATS | FL_XF | FL_FIN | FL_MEET | FL_STAMP) X(FL_STATS | FL_XF | FL_FIN | FL_GN1 | FL_MEET | FL_STAMP)   /* diagnostics: tools/fin_stamps.py */
#define FC_LEAN_FLAVOURS_1(X) X(0) X(FL_POSTOP) X(FL_XF) X(FL_STATS) X(FL_STATS | FL_XF)

// the k-step-quad (FL_W4) flavours exist for the one tile that feeds its weights from registers: M32N32K4 at 3x3; the Block-closing
// ones among them also in the whole-window form (FL_WW)
constexpr bool ww_flavour(int FL) { return (FL & FL_FIN) && (FL & FL_XF) && !(FL & (FL_CAT | FL_RES)); }
template <int FL>
static void add_lean3() {
    add_tiles<3, FL>(LeanTiles{});
    add_row<TILE_M32N32K4, 3, FL | FL_W4>();
    if constexpr (ww_flavour(FL)) add_row<TILE_M32N32K4, 3, FL | FL_W4 | FL_WW>();
}

// Block-closing (fused tail) GEOMETRY flavours: one per tile geometry of the dim-32 inference plan at 4x32x32 (DESIGN.md section 4 lists the launches
// behind each row), each as plain / + GroupNorm(1) partials / either with stamps, the register-fed rows also in the whole-window form.
// X(tile, weights, meeting, key); key = geo_key(statistics form, TB, TW, cpg, Tst), conv_dev.h.  A Block-closing launch of any other
// geometry runs on the lean flavour of its mask that reads the geometry at run time (FC_LEAN_FLAVOURS_3 above) -- not on the all-in-one
// kernel, which has no register-fed (FL_W4) form of the 32-row tile: it would sum those layers' products in another order, and be slower.
#define FC_FIN_GEOMS(X)                                                                   \
    X(TILE_M128N32, 0, FL_MEET, geo_key(GEO_FAST, 1, 16, 8, 8))        /* 32 ch @ 32x32 */  \
    X(TILE_M128N32, 0, FL_MEET, geo_key(GEO_FAST, 1, 16, 16, 2))       /* 64 ch @ 16x16 */  \
    X(TILE_M64N32K2, 0, FL_MEET, geo_key(GEO_FAST, 1, 16, 8, 4))       /* 32 ch @ 16x16 */  \
    X(TILE_M64N32K2, 0, 0, geo_key(GEO_FAST, 1, 8, 32, 1))             /* 128 ch @ 8x8, a whole group per tile */ \
    X(TILE_M32N32K4, FL_W4, FL_MEET, geo_key(GEO_FAST, 1, 8, 16, 2))   /* 64 ch @ 8x8 */    \
    X(TILE_M32N32K4, FL_W4, 0, geo_key(GEO_PAIR, 2, 4, 32, 1))         /* 128 ch @ 4x4, two samples per tile */ \
    X(TILE_M32N32K4, FL_W4, FL_MEET, geo_key(GEO_PAIR, 2, 4, 64, 2))   /* 256 ch @ 4x4: a group spans two column tiles */
#define FC_FIN_VARIANTS(Y) Y(0) Y(FL_GN1) Y(FL_STAMP) Y(FL_GN1 | FL_STAMP)
constexpr int kFinBase = FL_STATS | FL_XF | FL_FIN;
template <int TILE, int W4, int MEET, int GEO>
static void add_fin_geom() {
#define Y(V) add_row<TILE, 3, kFinBase | W4 | MEET | (V), 0, GEO>();
    FC_FIN_VARIANTS(Y)
#undef Y
    if constexpr (W4 != 0) {
#define Y(V) add_row<TILE, 3, kFinBase | W4 | FL_WW | MEET | (V), 0, GEO>();
        FC_FIN_VARIANTS(Y)
#undef Y
    }
}

// The step-closing flavour (conv_dev.h FL_STEP): final_res_block's closing launch of the dim-32 plan at 4x32x32 -- the first row of
// FC_FIN_GEOMS with the meeting, no GroupNorm(1) partials -- and its stamped twin.  Nothing else is instantiated with the bit, and a launch
// that asks for it (ConvFin::step) without matching the key is an error, never another kernel: the plan has dropped its final_conv and
// init_conv launches by then.
constexpr int kStepGeo = geo_key(GEO_FAST, 1, 16, 8, 8), kStepMask = kFinBase | FL_MEET;

// Block-OPENING (conv1) GEOMETRY flavours: the first convolution of every ResnetBlock of the same plan -- statistics of the raw output, in the
// up path also the concatenated skip and the fused res_conv output -- each also with stamps.  A Block's conv1 has the output geometry of its
// closing launch, so the keys are those of FC_FIN_GEOMS; only the (tile, mask, key) triples the plan's 19 conv1 launches use exist.
// X(tile, weights, mask, key)
constexpr int kConv1Up = FL_STATS | FL_CAT | FL_RES;
#define FC_CONV1_GEOMS(X)                                                                   \
    X(TILE_M128N32, 0, FL_STATS, geo_key(GEO_FAST, 1, 16, 8, 8))       /* downs.0.* */      \
    X(TILE_M128N32, 0, kConv1Up, geo_key(GEO_FAST, 1, 16, 8, 8))       /* ups.3.*, final_res_block */ \
    X(TILE_M128N32, 0, kConv1Up, geo_key(GEO_FAST, 1, 16, 16, 2))      /* ups.2.* */        \
    X(TILE_M64N32K2, 0, FL_STATS, geo_key(GEO_FAST, 1, 16, 8, 4))      /* downs.1.* */      \
    X(TILE_M64N32K2, 0, kConv1Up, geo_key(GEO_FAST, 1, 8, 32, 1))      /* ups.1.* */        \
    X(TILE_M32N32K4, FL_W4, FL_STATS, geo_key(GEO_FAST, 1, 8, 16, 2))  /* downs.2.* */      \
    X(TILE_M32N32K4, FL_W4, FL_STATS, geo_key(GEO_PAIR, 2, 4, 32, 1))  /* downs.3.* */      \
    X(TILE_M32N32K4, FL_W4, FL_STATS, geo_key(GEO_PAIR, 2, 4, 64, 2))  /* mid_block1, mid_block2 */ \
    X(TILE_M32N32K4, FL_W4, kConv1Up, geo_key(GEO_PAIR, 2, 4, 64, 2))  /* ups.0.* */

static std::mutex g_build_mu;     // build_rows() fills through g_fill: one caller at a time
static void build_rows(std::vector<PipeRow>& rows) {
    rows.clear();
    g_fill = &rows;
#define X(T, W4, MEET, GEO) add_fin_geom<T, W4, MEET, GEO>();
    FC_FIN_GEOMS(X)
#undef X
    add_row<TILE_M128N32, 3, kStepMask | FL_STEP, 0, kStepGeo>();
    add_row<TILE_M128N32, 3, kStepMask | FL_STEP | FL_STAMP, 0, kStepGeo>();
#define X(T, W4, MASK, GEO) add_row<T, 3, (MASK) | (W4), 0, 0, GEO>(); add_row<T, 3, (MASK) | (W4) | FL_STAMP, 0, 0, GEO>();
    FC_CONV1_GEOMS(X)
#undef X
    // (split-bf16: four staging waves as in the fp32 form: eight measured 364 against 380 images/s on the SD-VAE decode)
    add_tiles<1, FL_ALL, 1>(AllTiles{}); add_tiles<2, FL_ALL, 1>(AllTiles{}); add_tiles<3, FL_ALL, 1>(AllTiles{});
    add_tiles<1, FL_ALL>(AllTiles{}); add_tiles<2, FL_ALL>(AllTiles{}); add_tiles<3, FL_ALL>(AllTiles{}); add_tiles<5, FL_ALL>(AllTiles{});
#define X(F) add_lean3<(F)>();
    FC_LEAN_FLAVOURS_3(X)
#undef X
#define X(F) add_tiles<1, (F)>(LeanTiles{}); add_tiles<1, (F)>(Wide1Tiles{});
    FC_LEAN_FLAVOURS_1(X)
#undef X
    add_tiles<2, 0>(LeanTiles{});
    g_fill = &g_rows;
}

static const PipeRow* find_row(int tile, int ks, int fl, int prec = 0, int geof = 0, int geok1 = 0) {
    if (ks < 0 || ks >= 16) return nullptr;
    const unsigned long long key = pipe_key(tile, ks, fl, prec, geof, geok1);
    for (int i = g_begin[tile * 16 + ks]; i < g_begin[tile * 16 + ks + 1]; ++i)
        if (g_keys[i] == key) return &g_rows[i];
    return nullptr;
}

// The statistics geometry of a launch on `tile`, shared by the two kinds of geometry key: form, channels per group, column tiles and
// groups per tile, statistics slots per group (at most max_Tst).  False when the launch is not one a geometry flavour may take.
struct StatGeo { int BM, BN, nthr, form, cpg, ngt, Tst; };
static bool stat_geometry(const ConvDev& d, int tile, int max_Tst, StatGeo* g) {
    const ConvArgs& a = d.a;
    const TileInfo t = conv_tile_info(tile, true);
    if (!a.stats_out || a.par4 || a.stats_tmul != 1 || a.stats_toff != 0) return false;
    if (d.TB != 1 && d.TB != 2) return false;
    if (d.rps != t.BM / d.TB || (1 << (d.TWl + d.THl)) * d.TB != t.BM) return false;
    const bool pair_tile = t.BM == 32 && t.BN == 32;
    const int form = (pair_tile && d.TB == 2 && d.rps == 16) ? GEO_PAIR : (d.TB == 1 ? GEO_FAST : 0);
    if (!form) return false;
    const int cpg = d.cpg, NPG = cpg >= t.BN ? cpg / t.BN : 1;
    if (cpg < 1 || (cpg & (cpg - 1)) || cpg > (1 << 15) || d.cpgt != (cpg < t.BN ? cpg : t.BN) || d.NPG != NPG) return false;
    const int Tst = (d.TB > 1 ? 1 : d.tiles_x * d.tiles_y) * NPG;
    if (Tst < 1 || Tst > max_Tst) return false;
    *g = {t.BM, t.BN, 256 + 64 * conv_tile_nl(tile, 3), form, cpg, cpg >= t.BN ? 1 : t.BN / cpg, Tst};
    return true;
}

// The geometry key of a Block-closing launch, or 0 when the launch is not one a geometry flavour may take: the flavours assume (and
// compile in) everything tested here.
static int fin_geo_key(const ConvDev& d, int tile) {
    const ConvArgs& a = d.a;
    StatGeo g;
    if (!a.fin.gamma || a.s1.C || !a.s0.xf.mode || !stat_geometry(d, tile, kPartPre, &g)) return 0;
    if (a.Cout % g.BN || a.Cin != a.Cout || a.s0.xf.G <= 0 || a.s0.C != a.s0.xf.G * g.cpg || a.s0.xf.T != g.Tst) return 0;   // the input is this Block's own h
    if (d.TB * a.Cin > g.nthr - 256 || d.TB * a.s0.xf.G > g.nthr - 256 || d.TB * g.ngt * g.Tst * 2 > g.nthr) return 0;        // one table entry / granule per thread
    return geo_key(g.form, d.TB, 1 << d.TWl, g.cpg, g.Tst);
}

// The geometry key of a conv1 launch, or 0 when it is not one a conv1 geometry flavour may take: the statistics geometry as above, and
// besides it a plain 3x3 stride-1 window (no upsampling, no parity form, no activation or addend), kFinGeomGroups groups over whole
// column tiles and the wide store form.
static int conv1_geo_key(const ConvDev& d, int tile) {
    const ConvArgs& a = d.a;
    StatGeo g;
    if (a.fin.gamma || a.stats_post || d.any_xf || a.out_act || a.add || d.o_out < 0 || !stat_geometry(d, tile, 63, &g)) return 0;
    if (a.KS != 3 || a.stride != 1 || a.ups || a.pad != 1 || a.pad_y >= 0 || a.pad_x >= 0 || a.out_sh || a.out_oy || a.out_ox || a.Hs != a.H || a.Ws != a.W) return 0;
    if (a.Gout != kFinGeomGroups || a.Cout != kFinGeomGroups * g.cpg || a.Cout % g.BN || d.ntiles != a.Cout / g.BN) return 0;
    const int TW = 1 << d.TWl, TH = 1 << d.THl;
    if (d.PW != TW + 2 || d.PH != TH + 2 || d.P != d.TB * d.PH * d.PW) return 0;
    return geo_key(g.form, d.TB, TW, g.cpg, g.Tst);
}

static bool lean_kernels_on() {
    static const bool lean = [] { const char* e = std::getenv("FLOCODER_AMD_LEAN_KERNELS"); return !(e && std::string(e) == "0"); }();
    return lean;
}
bool conv_pipe_step_ok(const ConvDev& d, int tile) {
    const ConvArgs& a = d.a;
    return lean_kernels_on() && tile == TILE_M128N32 && a.KS == 3 && !d.bf3 && d.o_out >= 0 && !a.fin.gn1_out && !a.res_out && !a.stats_post && !a.out_act && !a.add &&
           !d.fin_local && d.any_xf && !a.out_sh && !a.out_oy && !a.out_ox && a.Cout == kStepDim && d.ntiles == 1 && conv_staging_fits(d.P, tile, 3, kLeanNPL) &&
           d.gsz == geo_Tst(kStepGeo) && fin_geo_key(d, tile) == kStepGeo;
}

// Whole-window staging (FL_WW): the LDS bytes of the launch in that form, or 0 when it keeps the per-chunk loader -- the window of all Cin
// chunks (chunk i at o_patch + i patch_stride; the tail's scratch aliases it as before) does not fit, a thread would hold more than
// kWWSlots elements, or the grid needs two workgroups per CU, which the larger LDS may not allow.  The caller has checked the
// register-fed form's own conditions (pipe_w4: whole 32-channel chunks, pad 1).
static int g_pipe_cus = 0;
static size_t ww_lds(const ConvDev& d, int tile, size_t lds) {
    const ConvArgs& a = d.a;
    if (tile != TILE_M32N32K4 || a.KS != 3 || !a.fin.gamma || a.s1.C || !a.s0.xf.mode || a.res_out || a.stride != 1) return 0;
    if ((long)d.P * (a.Cin / 4) > (long)kWWSlots * 768 || d.nblocks > g_pipe_cus) return 0;
    const size_t win = (size_t)(d.o_patch + d.nchunks * d.patch_stride) * sizeof(float), tot = win > lds ? win : lds;
    return tot <= 160 * 1024 ? tot : 0;
}

// The flavour mask of a launch: what the instantiation it runs on has to be able to do.  The selection and the occupancy cache both ask here.
static int pipe_need(const ConvDev& d, int tile) {
    const ConvArgs& a = d.a;
    return (a.fin.gamma ? FL_FIN : 0) | (a.res_out ? FL_RES : 0) | (a.stats_post ? FL_POST : 0) | (d.any_xf ? FL_XF : 0) |
           (a.s1.C ? FL_CAT : 0) | (d.stamps ? FL_STAMP : 0) | (a.stats_out ? FL_STATS : 0) | (a.fin.gn1_out ? FL_GN1 : 0) |
           ((a.out_act || a.add) ? FL_POSTOP : 0) | (d.o_out < 0 ? FL_NARROW : 0) |
           ((d.TB > 1 && tile != TILE_M32N32K4) ? FL_MULTI : 0) |        // (the 32-row tile always handles several samples)
           ((a.fin.gamma && !d.fin_local) ? FL_MEET : 0);
}
// register-fed weights in the k-step-quad layout: whole 32-channel chunks, whole 32-column tiles, the centre tap at (1, 1)
static bool pipe_w4(const ConvDev& d, int tile) {
    const ConvArgs& a = d.a;
    return tile == TILE_M32N32K4 && a.KS == 3 && a.w4 && a.Cin % 32 == 0 && a.Cout % 32 == 0 && a.pad == 1 && !a.w_batch_stride && (!a.res_out || a.res_w4);
}

// The row a launch runs on and the LDS bytes to launch it with (the whole-window form has its own).  With lean kernels on, the smallest
// flavour that covers the launch, in this order: the step-closing flavour (or its error), the flavour of exactly this geometry, the
// whole-window, k-step-quad and plain lean flavours of the mask; else the all-in-one kernel.
struct PipePick { const PipeRow* row; size_t lds; };
static int conv_pipe_select(const ConvDev& d, int tile, size_t lds, PipePick* out) {
    const ConvArgs& a = d.a;
    if (tile < 0 || tile >= TILE_COUNT) return fail(FC_E_ARG, "conv: bad tile id");
    if (d.bf3) {
        *out = {find_row(tile, a.KS, FL_ALL, 1), lds};
        return out->row ? FC_OK : fail(FC_E_ARG, "conv: no split-bf16 form of this tile");
    }
    // a lean row is taken if it exists and its loader can stage the window (the whole-window form has no per-chunk loader)
    auto take = [&](int fl, int geof, int geok1, size_t row_lds) {
        const PipeRow* r = find_row(tile, a.KS, fl, 0, geof, geok1);
        if (!r || (!(fl & FL_WW) && !conv_staging_fits(d.P, tile, a.KS, r->targ[A_NPL]))) return false;
        *out = {r, row_lds};
        return true;
    };
    const bool lean = lean_kernels_on();
    if (a.fin.step && !(lean && a.KS == 3)) return fail(FC_E_STATE, "conv: the step-closing flavour is a lean 3x3 kernel");
    if (lean) {
        const int need = pipe_need(d, tile), w4 = pipe_w4(d, tile) ? FL_W4 : 0;
        const size_t lds_ww = (w4 && (need & FL_FIN)) ? ww_lds(d, tile, lds) : 0;
        if ((need & FL_FIN) && a.fin.step) {
            if (conv_pipe_step_ok(d, tile) && (need & ~FL_STAMP) == kStepMask && take(need | FL_STEP, kStepGeo, 0, lds)) return FC_OK;
            return fail(FC_E_STATE, "conv: the launch is not the one the step-closing flavour is compiled for");
        }
        if (a.KS == 3 && (need & FL_FIN)) {             // Block-closing: whole-window where the launch may take it and the layer has the groups the flavour's trip counts assume
            const int geo = fin_geo_key(d, tile);
            if (geo && lds_ww && a.Cin == kFinGeomGroups * geo_cpg(geo) && take(need | w4 | FL_WW, geo, 0, lds_ww)) return FC_OK;
            if (geo && take(need | w4, geo, 0, lds)) return FC_OK;
        } else if (a.KS == 3 && (need & FL_STATS)) {    // Block-opening
            const int geo = conv1_geo_key(d, tile);
            if (geo && take(need | w4, 0, geo, lds)) return FC_OK;
        }
        if (lds_ww && take(need | FL_W4 | FL_WW, 0, 0, lds_ww)) return FC_OK;
        if (w4 && take(need | FL_W4, 0, 0, lds)) return FC_OK;
        if (take(need, 0, 0, lds)) return FC_OK;
    }
    *out = {find_row(tile, a.KS, FL_ALL), lds};
    return out->row ? FC_OK : fail(FC_E_SHAPE, "conv: kernel size not instantiated in the pipelined kernel");
}

bool conv_pipe_supports_ks(int ks) { return ks == 1 || ks == 2 || ks == 3 || ks == 5; }

// Once per process, before any launch or graph capture: the table, and the full 160 KiB of LDS for every row of it.
int conv_pipe_init() {
    static bool done = false;
    if (done) return FC_OK;
    std::lock_guard<std::mutex> lk(g_build_mu);
    build_rows(g_rows);
    std::sort(g_rows.begin(), g_rows.end(), [](const PipeRow& x, const PipeRow& y) { return x.key < y.key; });
    g_keys.clear();
    for (const PipeRow& r : g_rows) {
        if (!g_keys.empty() && g_keys.back() == r.key)      // two rows with one match key: the second could never be selected
            return fail(FC_E_STATE, "conv: two instantiations of the pipelined kernel share a match key");
        g_keys.push_back(r.key);
        FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(r.fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    for (int b = 0, i = 0; b <= kBuckets; ++b) {            // the key's bits above 48 are its bucket
        while (i < (int)g_keys.size() && (int)(g_keys[i] >> 49) < b) ++i;
        g_begin[b] = i;
    }
    int dev = 0;
    hipDeviceProp_t prop;
    FC_HIP(hipGetDevice(&dev));
    FC_HIP(hipGetDeviceProperties(&prop, dev));
    g_pipe_cus = prop.multiProcessorCount;
    FC_HIP(hipMalloc(reinterpret_cast<void**>(&g_zeros16), 256));
    FC_HIP(hipMemset(g_zeros16, 0, 256));
    done = true;
    return FC_OK;
}

// Diagnostics (fc_debug_conv_routes, tools/flavour_sizes.py): the thirteen template arguments of the instantiation every launch went to, one line
// per launch -- they are the instantiation's name in the code object's symbol table.
static std::mutex g_route_mu;
static bool g_route_on = false;
static std::string g_route_log;
void conv_route_log_set(bool on) { std::lock_guard<std::mutex> lk(g_route_mu); g_route_on = on; if (on) g_route_log.clear(); }
std::string conv_route_log_get() { std::lock_guard<std::mutex> lk(g_route_mu); return g_route_log; }

// Diagnostics (fc_debug_conv_table_read): every row of the table in the route record's format, one line of the thirteen template arguments per
// instantiation, in the order build_rows() names them.  Host code only -- build_rows() takes the addresses of the kernels' host stubs and
// nothing else -- so the listing needs neither conv_pipe_init() nor a device; it is built into a vector of its own, never into the table.
std::string conv_table_list() {
    std::vector<PipeRow> rows;
    {
        std::lock_guard<std::mutex> lk(g_build_mu);
        build_rows(rows);
    }
    std::string out;
    for (const PipeRow& r : rows)
        for (int i = 0; i < 13; ++i) out += std::to_string(r.targ[i]) + (i < 12 ? " " : "\n");
    return out;
}

int conv_pipe_launch(const ConvDev& d, int tile, int grid, size_t lds, hipStream_t s) {
    PipePick k;
    FC_TRY(conv_pipe_select(d, tile, lds, &k));
    if (k.row->targ[A_FL] & FL_STEP) step_route_log_add("step_close");
    if (g_route_on) {
        std::lock_guard<std::mutex> lk(g_route_mu);
        for (int i = 0; i < 13; ++i) g_route_log += std::to_string(k.row->targ[i]) + (i < 12 ? " " : "\n");
    }
    hipLaunchKernelGGL(k.row->fn, dim3(grid), dim3(k.row->nthr), k.lds, s, d);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// Workgroups of the instantiation this launch would go to that ONE CU holds at once (registers, waves and LDS as the runtime counts
// them; the fused tail's residency condition is derived from that, per instantiation -- conv_igemm.hip), cached per (tile, kernel size,
// flavour mask, LDS bytes, statistics geometry: a Block-closing launch's flavour depends on it).  0 = the query failed.
// A launch without a fused tail is asked for afresh: a conv1 launch's flavour also depends on what conv1_geo_key() tests (groups, window,
// stride, source extent), which the cache key does not hold.
static int pipe_query_blocks_per_cu(const ConvDev& d, int tile, size_t lds) {
    PipePick k;
    int occ = 0;
    if (conv_pipe_select(d, tile, lds, &k) != FC_OK) return 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k.row->fn, k.row->nthr, k.lds) == hipSuccess ? occ : 0;
}
int conv_pipe_blocks_per_cu(const ConvDev& d, int tile, size_t lds) {
    if (!d.a.fin.gamma) return pipe_query_blocks_per_cu(d, tile, lds);
    static std::map<std::tuple<int, int, int, size_t, int, int>, int> cache;
    static std::mutex mu;
    // (whether a launch takes the whole-window form depends on its grid and Cin as well: part of the key)
    const int ww = (d.a.KS == 3 && d.a.w4 && ww_lds(d, tile, lds)) ? d.a.Cin : 0;
    const auto key = std::make_tuple(tile, d.a.KS, pipe_need(d, tile) | (d.a.w4 ? FL_W4 : 0) | (d.a.fin.step ? FL_STEP : 0), lds, d.cpg,
                                     d.TB * 4096 + (d.TWl << 8) + d.tiles_x * d.tiles_y * d.NPG + (ww << 13));
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    return cache[key] = pipe_query_blocks_per_cu(d, tile, lds);
}

}  // namespace fc
