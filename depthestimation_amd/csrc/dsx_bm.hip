// bm2: fused block-matching pass for gfx950 (SURVEY.md 8a row A5'; replaces the arithmetic
// of cv2.StereoSGBM::compute called at depthlib/stereo_core.py:231).
//
// Work decomposition
//   * One block = NW waves = Dp disparities. SAD lanes own a disparity PAIR (d0, d0+1) whose
//     costs live in the two u16 halves of one VGPR (v_sad_u8 / v_sad_hi_u8 on zero-extended bytes
//     add an absolute difference into the low / high half, carry-free full-rate v_add/sub_u32
//     for the sums; SAD window sums <= 225*255 fit u16); SSD lanes own one disparity, summed
//     exactly in f32 (FSS below) or u32.
//   * The image is cut into vertical strips of TX = 32 output columns.  The (strip, row)
//     space is split over a persistent grid (blocks = resident capacity; host-computed
//     partition, bm2_partition), each block
//     sweeping down contiguous rows of a strip with running column sums (2 absolute
//     differences per column per row: the entering and the leaving row), so there is no
//     tail generation and no per-tile re-initialisation except at segment starts.
//   * Each row step needs the entering row (y+R+1) and the leaving row (y-R); both are staged
//     in double-buffered LDS slots.  The searched row is stored as one zero-extended dword per
//     entry, B[j] = src(pos(j)), in "disparity order" (j grows with d): a pair lane's two
//     disparities take neighbouring entries, and over a row it reads B[d0 .. d0+NC] with one
//     aligned ds_read_b64 per two columns (+ one dword); the reference row is wave-uniform: it is
//     stored as one zero-extended dword per column (f32 for FSS) and read with broadcast 16-B
//     LDS loads (4 columns each).  The next step's rows are prefetched from HBM into VGPRs
//     while the current row computes.
//   * Per row the TX x Dp costs go to an LDS tile; the epilogue re-reads it with TPP = 2*NW
//     lanes per pixel (DSL = Dp/TPP disparities each), finds the minimum with packed block
//     minima (8 disparities per 16-B read), the lowest winning d with a short scan of the
//     winning block, combines the TPP lanes with DPP quad_perm / ds_swizzle, and applies the
//     uniqueness test, the parabola sub-pixel and the left-right check.
//   side 0 (left)   : full epilogue -> int16 x16 + float disparity
//   side 1 (right)  : argmin only   -> right-view winners dR (LR check input)
//   side 2 (volume) : tile copied to the [H][W][Dp] cost volume (north-star "K1")
//   side 3 (left+LR): side 0 plus right-view winners built along the tile's cost diagonals
//                     (atomicMin across strips), checked afterwards by lr_fixup
//   side 4 (left+CV): side 0 plus OpenCV's LR keys (each unique winner offers (cost, d) to its right
//                     pixel), checked afterwards by lr_fixup_sgbm
#include "dsx_internal.h"
#include "dsx_partition.h"
#include "dsx_subpix.h"

// Register budget (waves per SIMD) the fused pass is compiled for, measured per cost (r01e): SAD at 4
// waves spills in the row loop (C2 +45 %); SSD blocks of >= 4 waves (D > 128) gain at 4 despite init
// spills (C3 392 -> 350 us); other SSD shapes were not measured and keep 3.
constexpr int kWpe = 3;     // waves per SIMD the fused pass is compiled for (SAD, and SSD below 4 waves)
constexpr int kWpeSsd = 4;  // SSD blocks of >= 4 waves

// Compile-time switches of bm2_segment, each =1 by default; =0 restores the previous form, which other sides and
// radii still run, for an A/B build (tools/variant_bm.sh -D<SWITCH>=0; tools/isa_same.py compares the code objects).
//   DSX_ROWSTEP_ATID      lane-indexed tile stores of the pair layout outside the LR pass
//   DSX_ROWSTEP_KEY2      key argmin of the pair layout's left pass up to R = 5; the rotated row loop needs it
//                         
//   DSX_ROWSTEP_MERGE     merged row staging, one load and one 16-B store per staged row (MRG)
//   DSX_ROWSTEP_COLGROUP  3-column group sums of the 9x9 and 3x3 rotated loops (CG; DESIGN 4.1,
//                         profiles/colgroup_isa.txt)
//   DSX_ROWSTEP_TAILSPLIT rotated loop's tail: both lanes of a pixel key half of the winning block (TSP; DESIGN 4.1,
//                         profiles/tailsplit_isa.txt)
//   DSX_ROWSTEP_BLOCKMIN  rotated loop's block keys: a block's minimum in two packed ops, v_pk_minimum3_f16 and
//                         v_pk_min_u16 (BMN; DESIGN 4.1, profiles/blockmin_isa.txt).  Declared in dsx_internal.h:
//                         the host's padding value goes with it
//   DSX_SEGSTART_AHEAD    transposed init: chunk q + 1's LDS reads in front of chunk q's SADs (IAH)
//   DSX_SEGSTART_BATCH    transposed init: every row's loads in one batch ahead of the transposes (IBT)
// Removed, last present in commit 70ab923 (measurements: DESIGN 4.4, profiles/*_ab.txt): the rejected forms
// DSX_ROWSTEP_PAIRTAIL, DSX_ROWSTEP_SREF, DSX_ROWSTEP_SARGS, DSX_ROWSTEP_STAGEAHEAD, DSX_SEGSTART_SPART and
// DSX_SEGSTART_ROW0; folded to on: DSX_ROWSTEP_OVERLAP, DSX_ROWSTEP_AHEAD, DSX_ROWSTEP_STORELATE, DSX_ROWSTEP_DIVQ.
#ifndef DSX_ROWSTEP_ATID
#define DSX_ROWSTEP_ATID 1
#endif
#ifndef DSX_ROWSTEP_KEY2
#define DSX_ROWSTEP_KEY2 1
#endif
#ifndef DSX_ROWSTEP_MERGE
#define DSX_ROWSTEP_MERGE 1
#endif
#ifndef DSX_ROWSTEP_COLGROUP
#define DSX_ROWSTEP_COLGROUP 1
#endif
#ifndef DSX_ROWSTEP_TAILSPLIT
#define DSX_ROWSTEP_TAILSPLIT 1
#endif
#ifndef DSX_SEGSTART_AHEAD
#define DSX_SEGSTART_AHEAD 1
#endif
#ifndef DSX_SEGSTART_BATCH
#define DSX_SEGSTART_BATCH 1
#endif
constexpr bool kRowstepAtid = DSX_ROWSTEP_ATID;
constexpr bool kRowstepKey2 = DSX_ROWSTEP_KEY2;
constexpr bool kRowstepMerge = DSX_ROWSTEP_MERGE;
constexpr bool kRowstepColgroup = DSX_ROWSTEP_COLGROUP;
constexpr bool kRowstepTailsplit = DSX_ROWSTEP_TAILSPLIT;
constexpr bool kSegstartAhead = DSX_SEGSTART_AHEAD;
constexpr bool kSegstartBatch = DSX_SEGSTART_BATCH;

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

namespace dsx {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// One 8-B LDS read that stays one: a volatile load in the LDS address space is not paired by the
// load/store optimiser, which otherwise merges two neighbouring ds_read_b64 into one ds_read2_b64
// (8 LDS-array cycles per wave against 2 + 2).  The address space must be named: a plain volatile
// pointer turns the read into a flat load.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x2 lds_read_b64(const uint8_t *p) {
    return *(const volatile __attribute__((address_space(3))) u32x2 *)p;
}

__device__ __forceinline__ u16x2 as2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as1(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ int clampi2(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t umin2(uint32_t a, uint32_t b) { return a < b ? a : b; }
// Packed u16 pairs summed with 32-bit v_add_u32 / v_sub_u32, which issue in 2 cycles against 4 for
// every v_pk_* op (tools/ubench3.hip).  Exact whenever no half carries or borrows: column sums
// (<= 255 (2R+1)) plus or minus one of their own terms, box sums (<= 57,375) plus one column sum,
// and results that are themselves non-negative sums.
__device__ __forceinline__ u16x2 add_sub2(u16x2 a, u16x2 p, u16x2 q) { return as2(as1(a) + as1(p) - as1(q)); }
// a * b + c on 24-bit signed operands (|a|, |b| <= 255 here): one full-rate v_mad_i32_i24
__device__ __forceinline__ int mad_i24(int a, int b, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// a + b + c in one v_add3_u32.  Written out: from the plain sum of three group sums per pixel hipcc shares partial
// sums between the pixels of a box phase (35 v_add_u32 + 5 v_add3_u32 in dependent runs instead of 32 independent ops).
__device__ __forceinline__ uint32_t add3_u32(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// c + (|a - b| summed over the 4 bytes << 16): with zero-extended bytes in a and b the absolute
// difference lands in the high u16 half of a packed pair (v_sad_u8 is the low half's form); both
// issue in 4.15 cycles (tools/ubench3.hip) against 2 v_pk_* + 2 v_add/sub_u32 for max - min.  The
// builtin (not inline asm) is an instruction the scheduler can see and move.
__device__ __forceinline__ uint32_t sad_hi_u8(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_sad_hi_u8(a, b, c);
}
// min(src of lane l-1, key) with lane 0 keeping key: one v_min_u32_dpp wave_shr:1 whose disabled lane
// (bound_ctrl off) keeps the tied key.  Written out because hipcc re-associates the builtin form into
// v_mov -1 + v_mov_dpp + v_min3 (3 VALU for the pair of slot minima instead of 2).  s_nop 1: the DPP
// source may have been written by the previous VALU (2 wait states on gfx9).
__device__ __forceinline__ uint32_t min_shr1(uint32_t src, uint32_t key) {
    asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %0 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(key) : "v"(src));
    return key;
}
// Eight lane-indexed LDS stores: lane l writes v[j] to M0[15:0] + OFF0 + j * STRIDE + 4 l (bytes, LDS
// address space), j = 0..7.  ds_write_addtid_b32 takes no address VGPR, so a store moves one source
// dword to the LDS instead of two, and the per-row base additions of the ds_write2_b32 form go.
// M0 is set inside the statement (one SALU op per eight stores), so nothing depends on the compiler
// leaving M0 alone between statements; s_nop 0: one wait state between an SALU write of M0 and an
// add-TID LDS instruction.  hipcc does not count LDS operations inside inline asm: in order within a
// wave, but a multi-wave block must drain lgkmcnt itself before its barrier (lds_drain below).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
template <int OFF0, int STRIDE>
__device__ __forceinline__ void lds_store8_addtid(uint32_t m0base, const uint32_t (&v)[8]) {
    static_assert(OFF0 >= 0 && OFF0 + 7 * STRIDE < 65536, "16-bit offset field");
    asm volatile("s_mov_b32 m0, %8\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %0 offset:%9\n\t"
                 "ds_write_addtid_b32 %1 offset:%10\n\t"
                 "ds_write_addtid_b32 %2 offset:%11\n\t"
                 "ds_write_addtid_b32 %3 offset:%12\n\t"
                 "ds_write_addtid_b32 %4 offset:%13\n\t"
                 "ds_write_addtid_b32 %5 offset:%14\n\t"
                 "ds_write_addtid_b32 %6 offset:%15\n\t"
                 "ds_write_addtid_b32 %7 offset:%16"
                 :
                 : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "s"(m0base),
                   "n"(OFF0), "n"(OFF0 + STRIDE), "n"(OFF0 + 2 * STRIDE), "n"(OFF0 + 3 * STRIDE), "n"(OFF0 + 4 * STRIDE),
                   "n"(OFF0 + 5 * STRIDE), "n"(OFF0 + 6 * STRIDE), "n"(OFF0 + 7 * STRIDE)
                 : "memory", "m0");
}
#pragma clang diagnostic pop
__device__ __forceinline__ void lds_drain() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ uint32_t lds_offset(const uint8_t *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)p;
}
__host__ __device__ constexpr int rnd16(int v) { return (v + 15) & ~15; }
template <int R, bool SSD, int NW>
struct Geo {
    static constexpr int TX = 32;
    static constexpr int NC = TX + 2 * R;     // column sums per lane (even)
    static constexpr int NG3 = NC - 2;        // 3-column group sums per lane (the forms that keep them: CG in bm2_segment)
    static constexpr int KD = SSD ? 1 : 2;    // disparities per lane
    static constexpr int LDW = 64 * KD;       // disparities per wave
    static constexpr int Dp = NW * LDW;
    static constexpr int NT = 64 * NW;
    static constexpr int TPP = NT / TX;       // epilogue lanes per pixel (2*NW)
    static constexpr int DSL = Dp / TPP;      // disparities per epilogue lane (64 SAD, 32 SSD)
    static constexpr int CB = SSD ? 4 : 2;    // cost bytes
    // 16 B of row padding (LDS banks; the SAD LR pass parks one exit key per wave there, NW <= 4)
    static constexpr int PITCH = Dp * CB + 16;
    static constexpr int NJ = NC + Dp;        // S entries per staged row
    static constexpr int REFW = rnd16(NC + 4);  // >= 4 * ceil(NC / 4)
    static constexpr int SROW = rnd16(NJ * 4 + 16);  // >= 16 * ceil(NJ / 4): whole-lane b128 stores
    static constexpr int MAXJ = (NJ + NT - 1) / NT;
    static constexpr int NB = DSL / 8;        // 8-disparity blocks per epilogue lane
    // reference row (broadcast reads): one dword per column (zero-extended byte, f32 for FSS)
    static constexpr int REFB = rnd16(4 * (NC + 8));
    static constexpr int SLOT = SROW + REFB;
    static constexpr int SMEM0 = 4 * SLOT + TX * PITCH;
    static constexpr int SMEM = SMEM0 > (2 * R + 1) * SLOT ? SMEM0 : (2 * R + 1) * SLOT;
    // SAD LR pass, per-wave region after SMEM: the 31 exits
    static constexpr int XRB = 128;
};

// Diagnostic build (-DDSX_STAMPS, libdsx_diag.so): per-phase s_memtime sums per block.
#ifdef DSX_STAMPS
#define DSX_STAMP(i)                                                                        \
    do {                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                  \
        uint64_t t_;                                                                        \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");          \
        __builtin_amdgcn_sched_barrier(0);                                                  \
        if ((i) > 0) ph[(i)-1] += t_ - t_prev;                                              \
        t_prev = t_;                                                                        \
    } while (0)
#else
#define DSX_STAMP(i) \
    do {             \
    } while (0)
#endif

// Workgroup barrier that orders LDS only: global loads (the next-row prefetch) stay in flight
// across it, unlike __syncthreads() which drains vmcnt as well.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Block-level LDS ordering: a single-wave block needs no barrier (a wave's LDS operations
// execute in order), only a compiler fence; multi-wave blocks use the LDS-only barrier.
template <int NW>
__device__ __forceinline__ void block_sync() {
    if constexpr (NW == 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
    } else {
        lds_barrier();
    }
}

template <int TPP>
__device__ __forceinline__ uint32_t gmin(uint32_t v) {
    if constexpr (TPP > 1) v = umin2(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
    if constexpr (TPP > 2) v = umin2(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
    if constexpr (TPP > 4) v = umin2(v, (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x101F));
    if constexpr (TPP > 8) v = umin2(v, (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x201F));
    return v;
}


typedef const __attribute__((address_space(1))) uint8_t gu8;    // global memory, named for ld()
typedef const __attribute__((address_space(1))) uint32_t gu32;

// One segment: strip x0, rows [yb, ye). FAST: every staged search position lies inside the
// image (one unaligned dword load per lane and row); otherwise replicate-clamped
// byte loads. All per-row state is in plain registers (no structs / arrays with runtime
// indices, which hipcc would demote to scratch).
// The LR pass's row loop re-reads the launch arguments from the kernarg segment every row (scalar
// loads through a pointer the compiler cannot hoist) instead of keeping them live across the loop,
// where the SGPR budget spilled them to VGPR lanes: one v_readlane (a VALU op) per reuse, ~70 per
// row step.
template <bool RELOAD>
__device__ __forceinline__ Bm2Args kargs_row(const Bm2Args &a) {
    if constexpr (RELOAD) {
        typedef __attribute__((address_space(4))) const Bm2Args KArgs;
        KArgs *p = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(p));
        return *(const Bm2Args *)p;  // loads stay scalar: the address space is inferred through the cast
    } else {
        return a;
    }
}

template <int R, bool SSD, int NW, int SIDE, bool FAST, bool ABS, bool LRFULL>
__device__ __forceinline__ void bm2_segment(const Bm2Args &a_in, uint8_t *smem, int x0, int yb, int ye, long fin, long fout,
                                            bool lr_on, int done0, const int (&pe)[3], int &qcur, int wvu
#ifdef DSX_STAMPS
                                            , uint64_t (&ph)[8], uint64_t &t_prev, uint64_t &nsteps
#endif
) {
    using G = Geo<R, SSD, NW>;
    constexpr int TX = G::TX, NC = G::NC, Dp = G::Dp, NT = G::NT, TPP = G::TPP, DSL = G::DSL, CB = G::CB,
                  PITCH = G::PITCH, NJ = G::NJ, SLOT = G::SLOT, NB = G::NB, NJ4 = (NJ + 3) / 4;
    constexpr int side = SIDE;
    // the LR pass reloads the launch arguments per segment too: values derived from them in the
    // segment prologue would otherwise be hoisted out of the block's segment loop and spilled
    const Bm2Args a = kargs_row<SIDE == 3>(a_in);
    // FSS: SSD sums in f32.  Squared differences, column sums and (offset) box sums are integers
    // below 2^24, so v_sub_f32 / v_fma_f32 / v_add_f32 (full rate, ~2 cycles) are exact and
    // replace the quarter-rate v_mad_i32_i24.  Box sums carry a +2^23 offset: for box < 2^23
    // (SSD R <= 5: 121 * 255^2 = 7.87M) the f32 value 2^23 + box has ulp 1 and its bit pattern is
    // OFF + box, monotone as u32, so the tile and the LR keys take the raw bits (OFF's set bits
    // lie above 23 + DB and leave the (C << DB | d) order intact); the epilogue subtracts OFF.
    // ABS (SAD1): SAD with the SSD layout (one disparity per lane, u32 column / box sums) for D <= 64,
    // where the packed pairs would leave half of the wave on padding disparities
    constexpr bool FSS = SSD && !ABS && R <= 5 && (SIDE == 0 || SIDE == 3 || SIDE == 4);
    constexpr bool SGK = SIDE == 4;  // left pass + OpenCV-form LR keys (lr_form 'sgbm' on the fused path)
    constexpr uint32_t OFF = FSS ? 0x4B000000u : 0u;
    // Columns per chunk of the column-sum loops (the staged words of one chunk are in flight
    // together).  With one dword per reference column the 8-column chunks spill in the LR pass and
    // the u32 / SAD1 builds, which sit at their register budgets: those take 4, like the FSS row loop.
    constexpr int CW = (!FSS && (SSD || SIDE == 3)) ? 4 : 8, NCH = (NC + CW - 1) / CW;
    typedef typename std::conditional<FSS, float, typename std::conditional<SSD, uint32_t, u16x2>::type>::type acc_t;
    uint8_t *tile = smem + 4 * SLOT;

    // The 4-wave SSD build (128 VGPRs) rebuilds the lane index per segment from the wave index (an
    // SGPR) and mbcnt, so tid-derived values are computed per segment instead of held (and spilled)
    // across the kernel: 0 B of scratch.  The other builds keep threadIdx.x - the rebuild measured
    // slower there (C2r +6 %, C1 +14 %: fewer VGPRs, different occupancy and schedule).
    constexpr bool LANE_RB = SSD && !ABS && NW >= 4;
    int ln = 0;
    if constexpr (LANE_RB)  // mbcnt inside the asm: not hoisted out of the segment loop
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    else
        ln = (int)threadIdx.x & 63;
    const int tid = LANE_RB ? (wvu << 6) + ln : (int)threadIdx.x;
    const int wv = LANE_RB ? wvu : tid >> 6;
    const int H = a.H, W = a.W, m = a.m, D = a.D;
    const int64_t stride = a.stride;
    const int d0 = SSD ? (wv * 64 + ln) : (wv * 128 + 2 * ln);
    const uint32_t padv = a.padv;
    // S index j -> search position: left  j = d + NC-1-c, pos = PB - j  (pos = x' - m - d)
    //                               right j = d + c,      pos = PB + j  (pos = x' + m + d)
    const int PB = side == 1 ? (x0 - R + m) : (x0 - R - m + NC - 1);
    const int sgn = side == 1 ? 1 : -1;

    // ---- raw row loads (registers) and their LDS stores ----
    // FAST: w0 = dword of 4 search bytes; SLOW: w0..w3 = finished S words
    constexpr int NC4 = (NC + 3) / 4;
    // Branch-free: every lane loads (positions clamped into the row), so no load sits under an
    // exec branch and the compiler never drains vmcnt inside the prefetch; st() stores only the
    // lanes that own staged words.
    // RL2: the row loop's second form - scalar row bases in ld, a prefetch on every
    // step and staging ahead of the step's output stores.  The pair layout takes it (C2 -9 %, C5
    // -8 %, C4 +4 % in flight, C2r +1 %); the one-disparity layouts measured slower with it (C3
    // 322.7 -> 330 us, C1 13.19 -> 13.24 us) and keep the first form.
    constexpr bool RL2 = !SSD;
    // RL2, FAST: the lane's byte offsets into the reference / searched row.  The row loop passes them
    // through an empty asm once per step (in place, no instruction): left loop-invariant, their zero
    // extensions are hoisted as 64-bit pairs and every load then pays a v_lshl_add_u64 for the 64-bit
    // address form instead of taking SGPR base + 32-bit VGPR offset.
    uint32_t ofs_r = (uint32_t)(x0 - R + 4 * min(tid, NC4 - 1));
    uint32_t ofs_s = side == 1 ? (uint32_t)(PB + 4 * min(tid, NJ4 - 1)) : (uint32_t)(PB - 4 * min(tid, NJ4 - 1) - 3);
    // MRG (pair layout, FAST copy, outside the LR pass): a staged row takes one load and one 16-B store.
    // Lanes tid < NJ4 own a searched dword as before, lanes NJ4 <= tid < NJ4 + NC4 a reference dword
    // (the rest repeat the last one and store nothing).  The two images have different bases, so a
    // lane holds a 64-bit base per segment and a row costs one 64-bit add (the wave-uniform row
    // offset) and one load.  Per-lane v_perm_b32 selectors bring both byte orders - searched entries
    // run down with the byte index in the left forms, reference columns up - to one zero-extending
    // unpack of four ops, and one ds_write_b128 with a per-lane address stores the row.  Per step:
    // 2 loads, 2 stores and 10 VALU fewer.  The builds at their register budget keep the two-load form: the
    // LR pass, and the volume pass and the 15x15 OpenCV-keys pass, which spill with the merged one (32 B
    // at R = 4, 8 B).
    constexpr bool MRG = kRowstepMerge && RL2 && FAST && SIDE != 3 && SIDE != 2 && !(SIDE == 4 && R >= 7);
    static_assert(!MRG || NJ4 + NC4 <= NT, "merged staging: a lane per staged dword");
    // CG (the unaligned-dword copy of the rotated 9x9 and 3x3 loops): 3-column group sums.  cs[c], c < NG3, holds
    // G3[c] = the sums of columns c, c + 1, c + 2 over the live rows, in both halves; the window is 3 x 3 (R = 4) or 1
    // (R = 1) of them.  A staged searched entry j is the 3-byte window {p(pos(j)), p(pos(j) + 1), p(pos(j) + 2), 0}
    // and a staged reference column c is {r(c), r(c + 1), r(c + 2), 0}: pos(c + i, d) = pos(c, d) + i, so one
    // v_sad_u8 of the two adds the three columns' terms of one row and disparity.  Same integers in another order:
    // a half of G3 is at most 3 * 9 * 255 = 6,885 and a half of a box sum 20,655, so no half carries.
    //   staging: a lane's four windows take six source bytes, its own dword and the next one in x.  For a searched
    //     lane that is lane tid - 1's dword (the entries run down with x); the reference lanes are ordered down as
    //     well, so one DPP move (wave_shr:1) per staged row serves both roles, and the four v_perm_b32 select from
    //     the two dwords.  The bytes no lane holds - past lane 0's and the first reference lane's dword - only
    //     reach entries 0, 1 and columns >= NG3, which nothing reads.
    //   row step: NG3 groups instead of NC columns, read at entries d0 + 2 .. d0 + NC.
    //   segment start: the init forms the single-column sums as before; G3 is summed from them once, in place.
    //   box phase: v[k] = G3[k] + G3[k + 3] + G3[k + 6] (R = 4), G3[k] (R = 1): no running sum.
    // The clamped copy keeps the single-column form; a segment is wholly one or the other.
    constexpr bool CG = kRowstepColgroup && MRG && SIDE == 0 && NW == 1 && (R == 4 || R == 1) && kRowstepKey2;
    constexpr int NCU = CG ? G::NG3 : NC;  // columns (groups) of the rotated loop's column update
    const bool m_s = tid < NJ4;
    const int m_r = CG ? max(NC4 - 1 - (tid - NJ4), 0) : min(tid - NJ4, NC4 - 1);  // reference dword of a non-search lane
    const uint8_t *m_base = m_s ? a.src + fin + ofs_s : a.ref + fin + (uint32_t)(x0 - R + 4 * m_r);
    const bool m_dn = m_s && side != 1;  // bytes 3, 2, 1, 0 -> words 0 .. 3
    // CG: bytes 0 .. 3 are the lane's dword, 4 .. 7 the next one in x
    const uint32_t m_sel0 = CG ? (m_dn ? 0x0C050403u : 0x0C020100u) : (m_dn ? 0x0C0C0C03u : 0x0C0C0C00u),
                   m_sel1 = CG ? (m_dn ? 0x0C040302u : 0x0C030201u) : (m_dn ? 0x0C0C0C02u : 0x0C0C0C01u),
                   m_sel2 = CG ? (m_dn ? 0x0C030201u : 0x0C040302u) : (m_dn ? 0x0C0C0C01u : 0x0C0C0C02u),
                   m_sel3 = CG ? (m_dn ? 0x0C020100u : 0x0C050403u) : (m_dn ? 0x0C0C0C00u : 0x0C0C0C03u);
    const uint32_t m_lane = m_s ? (uint32_t)(16 * tid) : (uint32_t)(G::SROW + 16 * m_r);  // byte offset in a slot
    auto ldm = [&](int r, uint32_t &w) __attribute__((always_inline)) {
        const int yy = clampi2(r, 0, H - 1);
        long ro = (long)yy * stride;
        asm("" : "+s"(ro));  // pinned to SGPRs: left free, the product is folded into one v_mad_u64_u32 per load
        w = *reinterpret_cast<const uint32_t *>(m_base + ro);
    };
    auto stm = [&](uint8_t *sp, uint32_t w) __attribute__((always_inline)) {
        // CG: lane tid - 1's dword (lane 0: zero); the lanes that store and their sources are all active
        const uint32_t nb = CG ? (uint32_t)__builtin_amdgcn_mov_dpp((int)w, 0x138, 0xF, 0xF, true) : 0u;
        if (tid < NJ4 + NC4)
            *reinterpret_cast<uint4 *>(sp) = make_uint4(__builtin_amdgcn_perm(nb, w, m_sel0), __builtin_amdgcn_perm(nb, w, m_sel1),
                                                        __builtin_amdgcn_perm(nb, w, m_sel2), __builtin_amdgcn_perm(nb, w, m_sel3));
    };
    auto ld = [&](int r, uint32_t &w0, uint32_t &w1, uint32_t &w2, uint32_t &w3, uint32_t &rf) __attribute__((always_inline)) {
        const int yy = clampi2(r, 0, H - 1);
        // The row base is wave-uniform and the lane's part a small non-negative offset (FAST:
        // x0 - R + 4 tr >= 0, PB - 4 tj - 3 >= 1, PB + 4 tj >= 0 by the segment's FAST test; clamped:
        // an index in [0, W-1]), added as an unsigned 32-bit value: the loads take the scalar-base
        // form.  The base is pinned to SGPRs - left free, hipcc folds the lane's part into a hoisted
        // 64-bit per-lane base and pays one v_mad_u64_u32 (yy * stride + base) per load and step.
        // (the address space is named again behind the asm, or the loads come out as flat loads)
        // Pair layout only (RL2): the one-disparity layouts keep per-lane 64-bit addresses.
        const uint8_t *srow_ = a.src + fin + (long)yy * stride;
        const uint8_t *rrow_ = a.ref + fin + (long)yy * stride;
        if constexpr (RL2) {
            asm("" : "+s"(srow_));
            asm("" : "+s"(rrow_));
        }
        typedef typename std::conditional<RL2, gu8, const uint8_t>::type row8;
        typedef typename std::conditional<RL2, gu32, const uint32_t>::type row32;
        typedef typename std::conditional<RL2, uint32_t, int>::type rix;
        row8 *srow = (row8 *)srow_, *rrow = (row8 *)rrow_;
        const int tr = min(tid, NC4 - 1);
        if constexpr (FAST) {
            if constexpr (RL2) {
                rf = *reinterpret_cast<row32 *>(rrow + ofs_r);
            } else {
                rf = *reinterpret_cast<row32 *>(rrow + x0 - R + 4 * tr);
            }
        } else {
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) v |= (uint32_t)rrow[(rix)clampi2(x0 - R + 4 * tr + q, 0, W - 1)] << (8 * q);
            rf = v;
        }
        if constexpr (FAST) {
            const int tj = min(tid, NJ4 - 1);
            row8 *p;
            if constexpr (RL2) {
                p = srow + ofs_s;
            } else {
                // The one-wave LR builds (at their register budget) add one int offset: (srow + PB) - 4 * tj
                // keeps a 64-bit -4 * tj live across the segments, which spilled there.
                p = side == 1 ? srow + PB + 4 * tj : (SIDE == 3 && NW == 1) ? srow + (PB - 4 * tj - 3) : srow + PB - 4 * tj - 3;
            }
            w0 = *reinterpret_cast<row32 *>(p);
            if constexpr (RL2) w1 = w2 = w3 = 0;  // st() rebuilds them from w0 (first form: the caller's zeros)
        } else {
            uint32_t v[4];
            // The one-wave SAD LR builds recompute 4 * tid per load: hoisted, the 4 clamped indices
            // below are held across the kernel.  C4 19.5k -> 21.5k
            // Mpix/s with 3 frames in flight, C2r +1.5 %; the R >= 6 and two-wave builds measured
            // slower with it (C5 -0.5 %, C1 at D = 140 with the checks +2.5 %: profiles/r04ai_*)
            int t4 = 4 * tid;
            if constexpr (!SSD && NW == 1 && SIDE == 3)
                asm volatile("" : "+v"(t4));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = min(t4 + q, NJ - 1);
                const int pp = PB + sgn * j;
                uint32_t t = srow[(rix)clampi2(pp, 0, W - 1)];
                if constexpr (FSS) t = __float_as_uint((float)t);
                v[q] = t;
            }
            w0 = v[0];
            w1 = v[1];
            w2 = v[2];
            w3 = v[3];
        }
    };
    auto st = [&](int sl, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t rf) __attribute__((always_inline)) {
        if (FSS && tid < NC4) {
            *reinterpret_cast<uint4 *>(smem + sl * SLOT + G::SROW + 16 * tid) =
                make_uint4(__float_as_uint((float)(rf & 0xFFu)), __float_as_uint((float)((rf >> 8) & 0xFFu)),
                           __float_as_uint((float)((rf >> 16) & 0xFFu)), __float_as_uint((float)(rf >> 24)));
        } else if (tid < NC4) {
            *reinterpret_cast<uint4 *>(smem + sl * SLOT + G::SROW + 16 * tid) =
                make_uint4(rf & 0xFFu, (rf >> 8) & 0xFFu, (rf >> 16) & 0xFFu, rf >> 24);
        }
        if constexpr (FAST) {
            const uint32_t dw = w0;  // byte k = entry 4 tid + k (right) / 4 tid + 3 - k (left)
            if (side == 1) {
                w0 = dw & 0xFFu; w1 = (dw >> 8) & 0xFFu; w2 = (dw >> 16) & 0xFFu; w3 = dw >> 24;
            } else if constexpr (FSS) {  // v_cvt_f32_ubyte{3,2,1,0}
                w0 = __float_as_uint((float)(dw >> 24)); w1 = __float_as_uint((float)((dw >> 16) & 0xFFu));
                w2 = __float_as_uint((float)((dw >> 8) & 0xFFu)); w3 = __float_as_uint((float)(dw & 0xFFu));
            } else {
                w0 = dw >> 24; w1 = (dw >> 16) & 0xFFu; w2 = (dw >> 8) & 0xFFu; w3 = dw & 0xFFu;
            }
        }
        if (tid < NJ4) *reinterpret_cast<uint4 *>(smem + sl * SLOT + 16 * tid) = make_uint4(w0, w1, w2, w3);
    };
    // st() of the pair layout's row loop (RL2, never f32), at sp = the lane's 16 bytes of the slot's
    // searched row (smem + sl * SLOT + 16 * tid).  Apart from st(), which the one-disparity layouts and
    // the init keep word for word: routed through one body, their instruction streams changed.
    auto st_at = [&](uint8_t *sp, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t rf) __attribute__((always_inline)) {
        if (tid < NC4)
            *reinterpret_cast<uint4 *>(sp + G::SROW) = make_uint4(rf & 0xFFu, (rf >> 8) & 0xFFu, (rf >> 16) & 0xFFu, rf >> 24);
        if constexpr (FAST) {
            const uint32_t dw = w0;
            if (side == 1) {
                w0 = dw & 0xFFu; w1 = (dw >> 8) & 0xFFu; w2 = (dw >> 16) & 0xFFu; w3 = dw >> 24;
            } else {
                w0 = dw >> 24; w1 = (dw >> 16) & 0xFFu; w2 = (dw >> 8) & 0xFFu; w3 = dw & 0xFFu;
            }
        }
        if (tid < NJ4) *reinterpret_cast<uint4 *>(sp) = make_uint4(w0, w1, w2, w3);
    };
    // reference pixels of slot sl, columns [c0, c0+CW): broadcast 16-B LDS reads
    auto ref_chunk = [&](int sl, int c0, uint32_t(&rw)[CW]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < CW; c += 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(smem + sl * SLOT + G::SROW + 4 * (c0 + c));
            rw[c] = v.x; rw[c + 1] = v.y; rw[c + 2] = v.z; rw[c + 3] = v.w;
        }
    };
    // FSS: 8 f32 reference pixels, two broadcast 16-B reads
    auto ref_chunkf = [&](int sl, int c0, float(&rw)[8]) __attribute__((always_inline)) {
        const uint4 v0 = *reinterpret_cast<const uint4 *>(smem + sl * SLOT + G::SROW + 4 * c0);
        const uint4 v1 = *reinterpret_cast<const uint4 *>(smem + sl * SLOT + G::SROW + 4 * c0 + 16);
        rw[0] = __uint_as_float(v0.x); rw[1] = __uint_as_float(v0.y); rw[2] = __uint_as_float(v0.z); rw[3] = __uint_as_float(v0.w);
        rw[4] = __uint_as_float(v1.x); rw[5] = __uint_as_float(v1.y); rw[6] = __uint_as_float(v1.z); rw[7] = __uint_as_float(v1.w);
    };
    // this lane's S words for columns [c0, c0+CW) of slot sl: sw[c] is column c0+c's entry for d0 and,
    // pair layout, sw[c+1] the one for d0+1 (CW+1 entries: aligned 8-B reads + 1 dword).  The left
    // form's entries run down with c, so they are stored reversed and the extra one (sw[0]) is the
    // previous chunk's last entry: nx carries it from chunk to chunk (read at c0 == 0).
    auto s_chunk = [&](int sl, int c0, uint32_t(&sw)[CW + 1], uint32_t &nx) __attribute__((always_inline)) {
        const uint8_t *base = smem + sl * SLOT + d0 * 4;
        if constexpr (side == 1) {
            if constexpr (SSD) {
#pragma unroll
                for (int c = 0; c < CW; ++c) sw[c] = *reinterpret_cast<const uint32_t *>(base + (c0 + c) * 4);
            } else {
                base = (const uint8_t *)__builtin_assume_aligned(base, 8);
#pragma unroll
                for (int c = 0; c < CW; c += 2) {
                    if (c0 + c < NC) {
                        const u32x2 v = lds_read_b64(base + (c0 + c) * 4);
                        sw[c] = v.x;
                        sw[c + 1] = v.y;
                    }
                }
                const int ce = NC - c0 < CW ? NC - c0 : CW;  // one past the chunk's last column
                sw[ce] = *reinterpret_cast<const uint32_t *>(base + (c0 + ce) * 4);
            }
        } else {
            if constexpr (SSD) {
#pragma unroll
                for (int c = 0; c < CW; ++c) sw[c] = *reinterpret_cast<const uint32_t *>(base + (NC - 1 - c0 - c) * 4);
            } else {
                // column c0+c: B[d0 + NC-1-c0-c] = sw[c+1] (d0) and B[d0 + NC-c0-c] = sw[c] (d0+1)
                base = (const uint8_t *)__builtin_assume_aligned(base, 8);
                sw[0] = c0 == 0 ? *reinterpret_cast<const uint32_t *>(base + NC * 4) : nx;
#pragma unroll
                for (int c = 1; c < CW; c += 2) {
                    if (c0 + c < NC) {
                        const u32x2 v = lds_read_b64(base + (NC - 1 - c0 - c) * 4);
                        sw[c + 1] = v.x;
                        sw[c] = v.y;
                        nx = v.x;
                    }
                }
            }
        }
    };
    // the pair's entries for column c0+c: e0 for d0, e1 for d0+1
    auto pair_e0 = [](const uint32_t(&sw)[CW + 1], int c) __attribute__((always_inline)) -> uint32_t {
        return side == 1 ? sw[c] : sw[c + 1];
    };
    auto pair_e1 = [](const uint32_t(&sw)[CW + 1], int c) __attribute__((always_inline)) -> uint32_t {
        return side == 1 ? sw[c + 1] : sw[c];
    };

    // ---- segment init: column sums over rows yb-R .. yb+R ----
    acc_t cs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cs[c] = acc_t(0);
    // Measured per instantiation (r02, tools/si_ab.sh, same box): C1 (R=2) 20.5 -> 19.5 us, C4 (R=2)
    // 57.3 -> 56.3 us, C5 (R=7) 610 -> 581 us.  The R=4 instantiation (C2) once ran 72.9 -> 79.0 us
    // with it, because its row loop then scheduled worse (full vmcnt drains); with the row loop's
    // staging ahead of its stores that no longer holds and R=4 gains as well (C2 60.6 -> 59.1 us,
    // C2r 98.5 -> 95.5 us).  The R=4 LR pass (C2r) still keeps the row-by-row init: at its
    // 168-VGPR budget the transposed form spills 24 B of values held across the segments.
    // SAD1 (ABS, one disparity per lane) takes the same transposed init with one v_sad_u8 per column
    // and row group (the pair's first entry only)
    constexpr bool SADINIT = ABS || R != 4 || SIDE != 3;
    if constexpr ((!SSD || ABS) && side != 1 && SADINIT) {
        // SAD (left / volume passes): rows in groups of 4, bytes transposed so that one v_sad_u8
        // sums a column's 4 row terms for one disparity: TP_g[j] = {P(j), P(j+1)} with P(j) the
        // group's 4 search bytes at position pos(j) (one per row), R_g[c] the 4 reference bytes
        // of column c.  Per column 2 v_sad_u8 per group instead of 2 absolute differences and an
        // add per row (C2 init 115 -> ~30 issue cycles per column).  Rows past 2R are zero in
        // both, so they add nothing.
        constexpr int NGR = (2 * R + 1 + 3) / 4;  // row groups
        constexpr int TPG = rnd16(NJ4 * 32);   // pair entries of a group (8 B each)
        constexpr int RG = rnd16(NC4 * 16);     // reference dwords of a group
        static_assert(NGR * (TPG + RG) <= G::SMEM, "transposed init rows must fit the block's LDS");
        // IBT: the groups unrolled, so the row tests are compile-time and no load sits under a branch, and every
        // row's loads (3 per row, 27 at R = 4; the accumulators are not live yet) issued in front of the first
        // transpose, pinned with sched_barrier(0): the segment start waits for one global round trip instead of one
        // per group.  Unaligned-dword copy up to R = 4 outside the volume and LR passes; the others gain scratch
        // with it (with group g + 1's loads in front of group g's transposes as well: DESIGN 4.4) and keep the loop.
        constexpr bool IBT = kSegstartBatch && FAST && R <= 4 && SIDE != 2 && SIDE != 3;
        block_sync<NW>();
        // byte loader in the FAST layout for both paths: w = bytes of entries 3, 2, 1, 0 (byte k =
        // entry 3 - k: positions PB - 4 tj - 3 .. PB - 4 tj), e = entry 4, rf = 4 reference bytes
        auto ldb = [&](int r, uint32_t &w, uint32_t &e, uint32_t &rf) __attribute__((always_inline)) {
            const int yy = clampi2(r, 0, H - 1);
            const uint8_t *srow = a.src + fin + (long)yy * stride;
            const uint8_t *rrow = a.ref + fin + (long)yy * stride;
            const int tj = min(tid, NJ4 - 1), tr = min(tid, NC4 - 1);
            if constexpr (IBT) {
                // batched loads: wave-uniform row bases pinned to SGPRs and the lane's part as an unsigned 32-bit
                // offset (ofs_s >= 1, ofs_r >= 0 by the segment's FAST test), as in ld: no 64-bit address pair per load
                const uint8_t *sb_ = srow, *rb_ = rrow;
                asm("" : "+s"(sb_));
                asm("" : "+s"(rb_));
                gu8 *ps = (gu8 *)sb_ + ofs_s;
                w = *reinterpret_cast<gu32 *>(ps);
                e = ps[-1];
                rf = *reinterpret_cast<gu32 *>((gu8 *)rb_ + ofs_r);
            } else if constexpr (FAST) {
                const uint8_t *pp = srow + PB - 4 * tj - 3;
                w = *reinterpret_cast<const uint32_t *>(pp);
                e = pp[-1];
                rf = *reinterpret_cast<const uint32_t *>(rrow + x0 - R + 4 * tr);
            } else {
                uint32_t v = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) v |= (uint32_t)srow[clampi2(PB - 4 * tj - q, 0, W - 1)] << (8 * (3 - q));
                w = v;
                e = srow[clampi2(PB - 4 * tj - 4, 0, W - 1)];
                v = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) v |= (uint32_t)rrow[clampi2(x0 - R + 4 * tr + q, 0, W - 1)] << (8 * q);
                rf = v;
            }
        };
        // a group's 4 rows, loaded (rows past 2R are zero) ...
        auto ildg = [&](int g, uint32_t(&w)[4], uint32_t(&e)[4], uint32_t(&rf)[4]) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (4 * g + r <= 2 * R) {
                    ldb(yb - R + 4 * g + r, w[r], e[r], rf[r]);
                } else {
                    w[r] = 0;
                    e[r] = 0;
                    rf[r] = 0;
                }
            }
        };
        // ... and transposed into the group's LDS rows
        auto itrg = [&](int g, const uint32_t(&w)[4], const uint32_t(&e)[4], const uint32_t(&rf)[4]) __attribute__((always_inline)) {
            // P(entry q) = {w0.byte(3-q), w1.byte(3-q), w2.byte(3-q), w3.byte(3-q)}, q = 0..3
            uint32_t P[5];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t b = 3 - q;
                const uint32_t lo = __builtin_amdgcn_perm(w[1], w[0], 0x0C0C0000u | ((4u + b) << 8) | b);
                const uint32_t hi = __builtin_amdgcn_perm(w[3], w[2], 0x0C0C0000u | ((4u + b) << 8) | b);
                P[q] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
            }
            {
                const uint32_t lo = __builtin_amdgcn_perm(e[1], e[0], 0x0C0C0400u);
                const uint32_t hi = __builtin_amdgcn_perm(e[3], e[2], 0x0C0C0400u);
                P[4] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
            }
            if (tid < NJ4) {
                uint4 *tp = reinterpret_cast<uint4 *>(smem + g * TPG + 32 * tid);
                tp[0] = make_uint4(P[0], P[1], P[1], P[2]);
                tp[1] = make_uint4(P[2], P[3], P[3], P[4]);
            }
            // R(column 4 tr + k) = {rf0.byte(k), rf1.byte(k), rf2.byte(k), rf3.byte(k)}
            if (tid < NC4) {
                uint32_t Rv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t lo = __builtin_amdgcn_perm(rf[1], rf[0], 0x0C0C0000u | ((4u + k) << 8) | (uint32_t)k);
                    const uint32_t hi = __builtin_amdgcn_perm(rf[3], rf[2], 0x0C0C0000u | ((4u + k) << 8) | (uint32_t)k);
                    Rv[k] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                }
                *reinterpret_cast<uint4 *>(smem + NGR * TPG + g * RG + 16 * tid) = make_uint4(Rv[0], Rv[1], Rv[2], Rv[3]);
            }
        };
        if constexpr (IBT) {
            uint32_t w[NGR][4], e[NGR][4], rf[NGR][4];
#pragma unroll
            for (int g = 0; g < NGR; ++g) ildg(g, w[g], e[g], rf[g]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < NGR; ++g) itrg(g, w[g], e[g], rf[g]);
        } else {
#pragma unroll 1
            for (int g = 0; g < NGR; ++g) {
                uint32_t w[4], e[4], rf[4];
                ildg(g, w, e, rf);
                itrg(g, w, e, rf);
            }
        }
        block_sync<NW>();
        // this lane's pair entry for column c: TP_g[d0 + NC - 1 - c] (8-B aligned); groups in a
        // runtime loop, columns unrolled (a full unroll of both hoists every LDS read and spills)
        const uint8_t *tb = smem + d0 * 8;
        {
        uint32_t ae[NC], ao[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) ae[c] = ao[c] = 0;
        // IAH: chunk q + 1's reads (4 pair entries and the broadcast reference dwords) issued in front of chunk q's
        // SADs, two register sets pinned with sched_barrier(0) as in the rotated row loop: only a group's first
        // chunk waits with a full drain.  Left to the scheduler, every read sits directly in front of its use
        // (18 drains per group at R = 4, the wave idle on LDS latency).
        // The R >= 6 builds (88 and more accumulators) gain scratch with it and keep the one-set loop.
        constexpr bool IAH = kSegstartAhead && R <= 5;
        if constexpr (IAH) {
#pragma unroll 1
            for (int g = 0; g < NGR; ++g) {
                uint32_t rv[2][4], p0[2][4], p1[2][4];
                auto ird = [&](auto qc) __attribute__((always_inline)) {
                    constexpr int q = decltype(qc)::value, c0 = 4 * q, t = q & 1;
                    const uint4 rr = *reinterpret_cast<const uint4 *>(smem + NGR * TPG + g * RG + 4 * c0);  // broadcast
                    rv[t][0] = rr.x; rv[t][1] = rr.y; rv[t][2] = rr.z; rv[t][3] = rr.w;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (c0 + c < NC) {
                            if constexpr (ABS) {
                                p0[t][c] = *reinterpret_cast<const uint32_t *>(tb + g * TPG + (NC - 1 - c0 - c) * 8);
                            } else {
                                const uint2 pr = *reinterpret_cast<const uint2 *>(tb + g * TPG + (NC - 1 - c0 - c) * 8);
                                p0[t][c] = pr.x;
                                p1[t][c] = pr.y;
                            }
                        }
                    }
                };
                auto isad = [&](auto qc) __attribute__((always_inline)) {
                    constexpr int q = decltype(qc)::value, c0 = 4 * q, t = q & 1;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (c0 + c < NC) {
                            ae[c0 + c] = __builtin_amdgcn_sad_u8(rv[t][c], p0[t][c], ae[c0 + c]);
                            if constexpr (!ABS) ao[c0 + c] = __builtin_amdgcn_sad_u8(rv[t][c], p1[t][c], ao[c0 + c]);
                        }
                    }
                };
                auto ichunk = [&](auto qc) __attribute__((always_inline)) {
                    constexpr int q = decltype(qc)::value;
                    if constexpr (q < NC4) {
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (q + 1 < NC4) ird(std::integral_constant<int, q + 1>{});
                        __builtin_amdgcn_sched_barrier(0);
                        isad(qc);
                    }
                };
                ird(std::integral_constant<int, 0>{});
                ichunk(std::integral_constant<int, 0>{}); ichunk(std::integral_constant<int, 1>{});
                ichunk(std::integral_constant<int, 2>{}); ichunk(std::integral_constant<int, 3>{});
                ichunk(std::integral_constant<int, 4>{}); ichunk(std::integral_constant<int, 5>{});
                ichunk(std::integral_constant<int, 6>{}); ichunk(std::integral_constant<int, 7>{});
                ichunk(std::integral_constant<int, 8>{}); ichunk(std::integral_constant<int, 9>{});
                ichunk(std::integral_constant<int, 10>{}); ichunk(std::integral_constant<int, 11>{});
                static_assert(NC4 <= 12, "column chunks of the transposed init");
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll 1
        for (int g = 0; g < NGR; ++g) {
#pragma unroll
            for (int q = 0; q < NC4; ++q) {
                const int c0 = 4 * q;
                const uint4 rr = *reinterpret_cast<const uint4 *>(smem + NGR * TPG + g * RG + 4 * c0);  // broadcast
                const uint32_t rv[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c0 + c < NC) {
                        if constexpr (ABS) {
                            const uint32_t p0 = *reinterpret_cast<const uint32_t *>(tb + g * TPG + (NC - 1 - c0 - c) * 8);
                            ae[c0 + c] = __builtin_amdgcn_sad_u8(rv[c], p0, ae[c0 + c]);
                        } else {
                            const uint2 pr = *reinterpret_cast<const uint2 *>(tb + g * TPG + (NC - 1 - c0 - c) * 8);
                            ae[c0 + c] = __builtin_amdgcn_sad_u8(rv[c], pr.x, ae[c0 + c]);
                            ao[c0 + c] = __builtin_amdgcn_sad_u8(rv[c], pr.y, ao[c0 + c]);
                        }
                    }
                }
            }
        }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if constexpr (ABS) cs[c] = ae[c];
            else cs[c] = as2(ae[c] | (ao[c] << 16));  // <= 255 (2R+1) < 2^16
        }
        if constexpr (CG) {  // the group sums, in place and ascending (cs[NG3], cs[NG3 + 1] are dead behind this)
#pragma unroll
            for (int c = 0; c < G::NG3; ++c) cs[c] = as2(as1(cs[c]) + as1(cs[c + 1]) + as1(cs[c + 2]));
        }
        }

    } else {
    // rows yb-R .. yb+R staged in slots 0..2R (may overlap the tile)
    block_sync<NW>();
    {
        // groups of IG rows in flight: bounds the init phase's VGPRs below the main loop's
        constexpr int IG = 3;
#pragma unroll 1
        for (int i0 = 0; i0 <= 2 * R; i0 += IG) {
            uint32_t iw[IG][5];
#pragma unroll
            for (int i = 0; i < IG; ++i)
                if (i0 + i <= 2 * R) ld(yb - R + i0 + i, iw[i][0], iw[i][1], iw[i][2], iw[i][3], iw[i][4]);
#pragma unroll
            for (int i = 0; i < IG; ++i)
                if (i0 + i <= 2 * R) st(i0 + i, iw[i][0], iw[i][1], iw[i][2], iw[i][3], iw[i][4]);
        }
    }
    block_sync<NW>();
#pragma unroll 1
    for (int i = 0; i <= 2 * R; ++i) {  // runtime loop: a full unroll makes compile time explode
        uint32_t nx = 0;
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            const int c0 = CW * q;
            uint32_t sw[CW + 1], rw[CW];
            float rf8[8];
            s_chunk(i, c0, sw, nx);
            if constexpr (FSS) ref_chunkf(i, c0, rf8);
            else ref_chunk(i, c0, rw);
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (c0 + c < NC) {
                    if constexpr (FSS) {
                        const float t = rf8[c] - __uint_as_float(sw[c]);
                        cs[c0 + c] = __builtin_fmaf(t, t, cs[c0 + c]);
                    } else if constexpr (ABS) {
                        cs[c0 + c] = __builtin_amdgcn_sad_u16(rw[c], sw[c], cs[c0 + c]);  // + |ref - src|
                    } else if constexpr (SSD) {
                        const int t = (int)rw[c] - (int)sw[c];
                        cs[c0 + c] += (uint32_t)__mul24(t, t);  // v_mul_i32_i24: |t| <= 255
                    } else {  // + |ref - src(d0)| in the low half, + |ref - src(d0+1)| in the high half
                        cs[c0 + c] = as2(sad_hi_u8(rw[c], pair_e1(sw, c), __builtin_amdgcn_sad_u8(rw[c], pair_e0(sw, c), as1(cs[c0 + c]))));
                    }
                }
            }
            // SSD: one chunk's LDS words in flight at a time (hoisting them all spilled at 4 waves)
            if constexpr (SSD) __builtin_amdgcn_sched_barrier(0);
        }
    }
    }
    block_sync<NW>();  // init rows (which overlap the tile) are consumed

    // tile padding: disparities >= D never win
    for (int q = tid; q < TX * (Dp - D); q += NT) {
        const int k = q / (Dp - D), d = D + (q - k * (Dp - D));
        if constexpr (SSD) *reinterpret_cast<uint32_t *>(tile + k * PITCH + d * 4) = padv + OFF;
        else *reinterpret_cast<uint16_t *>(tile + k * PITCH + d * 2) = (uint16_t)padv;
    }
    block_sync<NW>();

    const bool edge = side == 1 && (x0 + m < 0 || x0 + TX - 1 + m + Dp - 1 > W - 1);
    const bool dodd = !SSD && (D & 1);
    const bool lane_writes = d0 < D;

    // RL2: the lane's bytes in slot par ^ 2 of the first step
    uint32_t stg = (MRG ? m_lane : (uint32_t)(16 * tid)) + (uint32_t)((2 - (yb & 1) * 2) * SLOT);
    // DIVQ (pair layout, left pass): the tail's sub-pixel quotient by subpix_quot (dsx_subpix.h); the other tails keep
    // div_trunc_small and its two divergent fix-up branches.
    constexpr bool DIVQ = !SSD && SIDE == 0;
    // OVL (pair layout, one-wave left pass, key argmin: R <= 5): the row loop rotated by half a step.  The
    // epilogue of row y - 1 reads only the tile, the column update of row y only the staged slots and the
    // column sums, and the tile is not rewritten before row y's box phase, so step y runs the two together:
    // the epilogue is cut into stages at its dependent LDS reads (the eight block reads, the winning block, the
    // two neighbour costs, the sub-pixel step) and stage s is issued in front of column chunk s, with one chunk
    // of SADs between a read and its first use.  sched_barrier(0) pins the pieces in source order.  The stages
    // are branch-free (the neighbour costs are read for every pixel and dropped where no step applies); the
    // wave-uniform uniqueness and parabola-float branches follow the last chunk.
    // A segment's first step has no epilogue and one epilogue drains the segment behind its last step.
    // The column update runs in 4-column chunks with chunk q + 1's LDS reads issued in front of chunk q's SADs, in
    // two register sets (only a step's first chunk waits), which together hold what one 8-column chunk does.
    // The two output stores of row y - 1 stand at the end of step y, behind the staging of step y + 1's rows: behind
    // the last chunk they would be older than the staging's loads, and vmcnt counts loads and stores in order, so the
    // staging would wait for a store round trip per step.  The outputs (the x16 value, the parabola float) are held
    // across the box phase in e_fx / e_pf, and the next wait that counts the stores is the next step's staging.
    constexpr bool OVL = !SSD && SIDE == 0 && NW == 1 && R < 6 && kRowstepKey2;
    int e_fx = 0;
    float e_pf = 0.0f;
    static_assert(!CG || OVL, "group sums: the rotated loop");
    constexpr int CQ = 4, NQ = (NCU + CQ - 1) / CQ;
    // BMN: a block's minimum (emin8 below) in two packed ops instead of three, v_pk_minimum3_f16 of three of its words
    // and one v_pk_min_u16 with the fourth (block_min8, dsx_internal.h): every cost of these kernels, the padding
    // included (the host's kBlockminPad), is below 0x7C00.  The keys are folded as before: hipcc already takes the
    // running key and two block keys in one v_min3_u32.
    constexpr bool BMN = kRowstepBlockmin && OVL;
    static_assert(!BMN || 255 * (2 * R + 1) * (2 * R + 1) < 0x7C00, "block minima as f16 bit patterns: finite costs only");
    // Tile reads per stage and read stages: one read (4 VGPRs in flight) where the chunks suffice, two otherwise.
    // With two, R = 4 and R = 5 spilled 8 B (again with BMN); four overran the 168 VGPRs even without
    // the reads ahead.
    // Stages 0 .. NRS - 1 read, NRS block keys, NRS + 1 element keys, NRS + 2 sub-pixel step, NRS + 3 outputs.
    constexpr int RPS = NQ >= 10 ? 1 : 2, NRS = 8 / RPS;
    static_assert(NQ >= NRS + 2, "a column chunk per stage up to the element keys");
    const int ek = tid / TPP, eh = tid % TPP, ex = x0 + ek;
    const uint8_t *epx = tile + ek * PITCH + eh * DSL * CB;
    // TSP: the winning block is read and keyed by both lanes of its pixel, four elements each.  The pair-combined
    // block key names the block for both, so lane eh reads the 8 bytes at 16 egblk + 8 eh of the pixel's tile row
    // (inside the row for egblk <= 15), forms four element keys (cost << 16 | element 0 .. 3), ors its half's
    // 4 eh into the free bit 2 and the pair's minimum carries the element 0 .. 7: lowest cost, then lowest element,
    // as before.  The lane that does not own the block keys no block that cannot win, and the owner select goes.
    constexpr bool TSP = kRowstepTailsplit && OVL;
    const uint8_t *ehx = tile + ek * PITCH + 8 * eh;
    const uint32_t eh4 = (uint32_t)(eh << 2);
    uint4 etv[2] = {};
    uint32_t ekmin = 0, ecb = 0, egblk = 0, ecm = 0, ecp = 0;
    int eb = 0, ef = 0, eden = 1;
    bool esp = false;
    auto emin8 = [](uint4 v) __attribute__((always_inline)) -> uint32_t { return block_min8<BMN>(v); };
    // the two output stores of a row, apart from the stage that forms the outputs where that stage defers them
    // ea: the row loop's own copy of the launch arguments.  Taken from the segment's copy (a) the same values come
    // out as another instruction stream (tools/isa_same.py: bm2<R, SAD, 1, 0>, R <= 5).
    auto estore = [&](int ey, const Bm2Args &ea) __attribute__((always_inline)) {
        if (eh == 0 && ex < W) {
            const long o = fout + (long)ey * W + ex;
            if (ea.out_fixed) ea.out_fixed[o] = (int16_t)e_fx;
            if (ea.out_float) ea.out_float[o] = ea.float_mode == 0 ? (float)(int16_t)e_fx * 0.0625f : e_pf;
        }
    };
    // dfr: the output stage leaves its stores to estore (the row loop; the drain behind a segment stores at once)
    auto estage = [&](auto sc, int ey, auto dfr) __attribute__((always_inline)) {
        constexpr int s = decltype(sc)::value;
        constexpr bool DFR = decltype(dfr)::value;
        static_assert(!OVL || (NB == 8 && TPP == 2), "overlapped epilogue: 64 disparities per lane, two lanes per pixel");
        constexpr int GB = Dp / 8 <= 16 ? 4 : (Dp / 8 <= 32 ? 5 : 6);
        if constexpr (s <= NRS) {  // RPS block reads per stage; the block keys (KEY2 of the sequential form) of those before
            if constexpr (s == 0) ekmin = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < (s > 0 ? RPS : 0); ++j) ekmin = umin2(ekmin, (emin8(etv[j]) << GB) | (uint32_t)(RPS * (s - 1) + j));
            if constexpr (s < NRS) {
#pragma unroll
                for (int j = 0; j < RPS; ++j) etv[j] = *reinterpret_cast<const uint4 *>(epx + 16 * (RPS * s + j));
            } else {  // the winning block and its read
                const uint32_t kmin = gmin<TPP>(ekmin | (uint32_t)(eh * 8));
                ecb = kmin >> GB;
                egblk = kmin & ((1u << GB) - 1u);
                if constexpr (TSP) {  // this lane's half of the pair's winning block
                    const uint2 v = *reinterpret_cast<const uint2 *>(ehx + 16 * egblk);
                    etv[0].x = v.x;
                    etv[0].y = v.y;
                } else {
                    etv[0] = *reinterpret_cast<const uint4 *>(epx + 16 * (egblk & 7u));
                }
            }
        } else if constexpr (s == NRS + 1) {  // element keys, the winner, its neighbours' reads
            if constexpr (TSP) {
                const uint32_t w0 = etv[0].x, w1 = etv[0].y;
                const uint32_t k4 = umin2(umin2(w0 << 16, (w0 & 0xFFFF0000u) | 1u),
                                          umin2((w1 << 16) | 2u, (w1 & 0xFFFF0000u) | 3u));
                eb = (int)(egblk * 8 + (gmin<TPP>(k4 | eh4) & 7u));
            } else {  // the owner lane keys all eight elements of its block
                const uint32_t w4[4] = {etv[0].x, etv[0].y, etv[0].z, etv[0].w};
                uint32_t k8 = 0xFFFFFFFFu;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    k8 = umin2(k8, (w4[q] << 16) | (uint32_t)(2 * q));
                    k8 = umin2(k8, (w4[q] & 0xFFFF0000u) | (uint32_t)(2 * q + 1));
                }
                const uint32_t dl = (int)(egblk / 8) == eh ? egblk * 8 + (k8 & 7u) : 0xFFFFu;
                eb = (int)gmin<TPP>(dl);
            }
            // b - 1 >= -1 and b + 1 <= Dp stay inside the block's LDS: the slot bytes before the tile, the row's padding
            const uint16_t *pc = reinterpret_cast<const uint16_t *>(tile + ek * PITCH) + eb;
            ecm = pc[-1];
            ecp = pc[1];
        } else if constexpr (s == NRS + 2) {  // sub-pixel step
            esp = a.subpix && eb > 0 && eb < D - 1;
            int32_t den = (int32_t)ecm + (int32_t)ecp - 2 * (int32_t)ecb;
            eden = den < 1 ? 1 : den;
            const int32_t num = ((int32_t)ecm - (int32_t)ecp) * 16 + eden;
            const int32_t q = subpix_quot(num, 2 * eden);  // for every pixel: the stage stays branch-free
            ef = eb * 16 + (esp ? q : 0);
        } else {  // uniqueness, outputs
            bool valid = ex < W && ex >= m + D - 1 && ex <= W - 1 + m;
            if (a.uniq > 0) {
                const int rel = eb - eh * DSL;
                uint32_t nm = 0xFFFFFFFFu;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    // the block minima are not held across the column update (8 VGPRs): read again
                    const bool hit = rel >= 8 * i - 1 && rel <= 8 * i + 8;
                    nm = hit ? nm : umin2(nm, emin8(*reinterpret_cast<const uint4 *>(epx + 16 * i)));
                }
                const int ib0 = (rel - 1) >> 3, ib1 = (rel + 1) >> 3;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int ib = t == 0 ? ib0 : ib1;
                    if (ib >= 0 && ib < 8 && (t == 0 || ib1 != ib0)) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(epx + 16 * ib);
                        const uint32_t c8[8] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16,
                                                v.z & 0xFFFFu, v.z >> 16, v.w & 0xFFFFu, v.w >> 16};
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int dd = 8 * ib + e - rel;
                            nm = (dd > 1 || dd < -1) ? umin2(nm, c8[e]) : nm;
                        }
                    }
                }
                nm = gmin<TPP>(nm);
                const uint32_t real_max = padv < (1u << 24) ? padv : (1u << 24);
                if (nm < real_max && nm * (uint32_t)(100 - a.uniq) < ecb * 100u) valid = false;
            }
            if constexpr (DFR) {
                e_fx = valid ? (int16_t)(m * 16 + ef) : (int16_t)((m - 1) * 16);
                if (eh == 0 && ex < W && a.out_float && a.float_mode != 0) {
                    float pf = (float)(m + eb);
                    if (esp) pf = (float)(m + eb) + (float)((int32_t)ecm - (int32_t)ecp) / (float)(2 * eden);
                    e_pf = valid ? pf : (float)(m - 1);
                }
            } else if (eh == 0 && ex < W) {
                const long o = fout + (long)ey * W + ex;
                const int16_t fx = valid ? (int16_t)(m * 16 + ef) : (int16_t)((m - 1) * 16);
                if (a.out_fixed) a.out_fixed[o] = fx;
                if (a.out_float) {
                    if (a.float_mode == 0) {
                        a.out_float[o] = (float)fx * 0.0625f;
                    } else {
                        float pf = (float)(m + eb);
                        if (esp) pf = (float)(m + eb) + (float)((int32_t)ecm - (int32_t)ecp) / (float)(2 * eden);
                        a.out_float[o] = valid ? pf : (float)(m - 1);
                    }
                }
            }
        }
    };
    for (int y = yb; y < ye; ++y) {
        const Bm2Args &a = kargs_row<SIDE == 3>(a_in);
#ifdef DSX_STAMPS
        ++nsteps;
#endif
        DSX_STAMP(0);
        if (a.prio) {
            // issue priority by progress quartile: waves that are behind (the younger ones on a
            // SIMD, which lose age arbitration) take the VALU first, so co-resident waves finish
            // together instead of leaving the last one alone on its SIMD
            // sign bits, not compares: the sum of three wave-uniform bools came out as v_cndmask +
            // v_readfirstlane pairs; (pe - 1 - dn) >> 31 stays on the scalar unit (|values| < 2^30)
            const int dn = done0 + (y - yb);
            // Pair layout only: with it C3 (bm2<5, SSD, 4, 3>) ran 321.4 -> 324.5 us, so the
            // one-disparity layouts keep the compares and their instruction streams.
            const int q = RL2 ? (int)(((uint32_t)(pe[0] - 1 - dn) >> 31) + ((uint32_t)(pe[1] - 1 - dn) >> 31) +
                                      ((uint32_t)(pe[2] - 1 - dn) >> 31))
                              : (dn >= pe[0]) + (dn >= pe[1]) + (dn >= pe[2]);
            if (q != qcur) {
                qcur = q;
                switch (q) {
                    case 0: __builtin_amdgcn_s_setprio(3); break;
                    case 1: __builtin_amdgcn_s_setprio(2); break;
                    case 2: __builtin_amdgcn_s_setprio(1); break;
                    default: __builtin_amdgcn_s_setprio(0); break;
                }
            }
        }
        if constexpr (RL2 && FAST && !MRG) asm volatile("" : "+v"(ofs_r), "+v"(ofs_s));
        const int par = (y & 1) * 2;  // slots {par, par+1} = {new row y+R, old row y-R-1}
        const bool more = y + 1 < ye;
        // prefetch the next step's entering / leaving rows (+ its dR segment); lands during this step.
        // RL2: issued on every step, the segment's last one included - ld clamps the row into
        // [0, H-1], so that step loads a valid row which nobody stores, and the zero initialisers
        // are dead.  First form (!RL2): under `if (more)`; writing the zeros then waits for the
        // previous step's loads and stores (s_waitcnt vmcnt(0) at the loop header).
        uint32_t pn0 = 0, pn1 = 0, pn2 = 0, pn3 = 0, pnr = 0, po0 = 0, po1 = 0, po2 = 0, po3 = 0, por = 0;
        if constexpr (MRG) {
            ldm(y + 1 + R, pn0);
            ldm(y - R, po0);
        } else if (RL2 || more) {
            ld(y + 1 + R, pn0, pn1, pn2, pn3, pnr);
            ld(y - R, po0, po1, po2, po3, por);
        }
        if constexpr (FSS) {
          if (y > yb) {
            // chunks of 4 columns (one broadcast b128 of reference pixels per slot): half the
            // transient registers of the 8-column chunks, which spilled at 4 waves / SIMD
#pragma unroll
            for (int q = 0; q < (NC + 3) / 4; ++q) {
                const int c0 = 4 * q;
                const uint4 rn = *reinterpret_cast<const uint4 *>(smem + par * SLOT + G::SROW + 4 * c0);
                const uint4 ro = *reinterpret_cast<const uint4 *>(smem + (par + 1) * SLOT + G::SROW + 4 * c0);
                const float rn4[4] = {__uint_as_float(rn.x), __uint_as_float(rn.y), __uint_as_float(rn.z), __uint_as_float(rn.w)};
                const float ro4[4] = {__uint_as_float(ro.x), __uint_as_float(ro.y), __uint_as_float(ro.z), __uint_as_float(ro.w)};
                const uint8_t *bn = smem + par * SLOT + d0 * 4, *bo = smem + (par + 1) * SLOT + d0 * 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c0 + c < NC) {
                        const float sn = *reinterpret_cast<const float *>(bn + (NC - 1 - c0 - c) * 4);
                        const float so = *reinterpret_cast<const float *>(bo + (NC - 1 - c0 - c) * 4);
                        // cs + tn^2 - to^2: two v_sub_f32 + two v_fma_f32 (neg modifier)
                        const float tn = rn4[c] - sn, to = ro4[c] - so;
                        cs[c0 + c] = __builtin_fmaf(-to, to, __builtin_fmaf(tn, tn, cs[c0 + c]));
                    }
                }
            }
          }
        } else if constexpr (OVL) {
          if (y > yb) {
            // this lane's staged words of chunk q (columns [CQ q, CQ q + CQ)), both slots: s_chunk / ref_chunk
            // of the left form at the chunk width of this path, in register set q & 1
            uint32_t sn[2][CQ + 1], so[2][CQ + 1], rn[2][CQ], ro[2][CQ];
            uint32_t nxn = 0, nxo = 0;
            auto rd = [&](auto qc) __attribute__((always_inline)) {
                constexpr int q = decltype(qc)::value, c0 = CQ * q, t = q & 1;
                const uint8_t *bn = (const uint8_t *)__builtin_assume_aligned(smem + par * SLOT + d0 * 4, 8);
                const uint8_t *bo = (const uint8_t *)__builtin_assume_aligned(smem + (par + 1) * SLOT + d0 * 4, 8);
                const uint4 vn = *reinterpret_cast<const uint4 *>(smem + par * SLOT + G::SROW + 4 * c0);
                const uint4 vo = *reinterpret_cast<const uint4 *>(smem + (par + 1) * SLOT + G::SROW + 4 * c0);
                rn[t][0] = vn.x; rn[t][1] = vn.y; rn[t][2] = vn.z; rn[t][3] = vn.w;
                ro[t][0] = vo.x; ro[t][1] = vo.y; ro[t][2] = vo.z; ro[t][3] = vo.w;
                sn[t][0] = c0 == 0 ? *reinterpret_cast<const uint32_t *>(bn + NC * 4) : nxn;
                so[t][0] = c0 == 0 ? *reinterpret_cast<const uint32_t *>(bo + NC * 4) : nxo;
#pragma unroll
                for (int c = 1; c < CQ; c += 2) {
                    if (c0 + c < NCU) {
                        const u32x2 pn = lds_read_b64(bn + (NC - 1 - c0 - c) * 4);
                        const u32x2 po = lds_read_b64(bo + (NC - 1 - c0 - c) * 4);
                        sn[t][c + 1] = pn.x; sn[t][c] = pn.y; nxn = pn.x;
                        so[t][c + 1] = po.x; so[t][c] = po.y; nxo = po.x;
                    }
                }
            };
            auto sads = [&](auto qc) __attribute__((always_inline)) {
                constexpr int q = decltype(qc)::value, c0 = CQ * q, t = q & 1;
#pragma unroll
                for (int c = 0; c < CQ; ++c) {
                    if (c0 + c < NCU) {
                        const uint32_t bn = rn[t][c], bo = ro[t][c];
                        const uint32_t en = sad_hi_u8(bn, sn[t][c], __builtin_amdgcn_sad_u8(bn, sn[t][c + 1], as1(cs[c0 + c])));
                        const uint32_t lo = sad_hi_u8(bo, so[t][c], __builtin_amdgcn_sad_u8(bo, so[t][c + 1], 0u));
                        // pinned to this chunk (in place, no instruction): left free, the SADs - pure values whose
                        // next use is the box phase - are sunk behind the epilogue's branches, every staged
                        // word of the step is then held across it, and the loop spills
                        uint32_t v = en - lo;
                        asm volatile("" : "+v"(v));
                        cs[c0 + c] = as2(v);
                    }
                }
            };
            // epilogue stage q and chunk q + 1's reads in front of chunk q
            auto chunk = [&](auto qc) __attribute__((always_inline)) {
                constexpr int q = decltype(qc)::value;
                if constexpr (q < NQ) {
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (q < NRS + 3) estage(qc, y - 1, std::false_type{});
                    if constexpr (q + 1 < NQ) rd(std::integral_constant<int, q + 1>{});
                    __builtin_amdgcn_sched_barrier(0);
                    sads(qc);
                }
            };
            rd(std::integral_constant<int, 0>{});
            chunk(std::integral_constant<int, 0>{}); chunk(std::integral_constant<int, 1>{});
            chunk(std::integral_constant<int, 2>{}); chunk(std::integral_constant<int, 3>{});
            chunk(std::integral_constant<int, 4>{}); chunk(std::integral_constant<int, 5>{});
            chunk(std::integral_constant<int, 6>{}); chunk(std::integral_constant<int, 7>{});
            chunk(std::integral_constant<int, 8>{}); chunk(std::integral_constant<int, 9>{});
            chunk(std::integral_constant<int, 10>{}); chunk(std::integral_constant<int, 11>{});
            static_assert(NQ <= 12 && NQ >= 7, "chunks of the overlapped column update");
            __builtin_amdgcn_sched_barrier(0);
            // the stages no chunk was left for; the outputs are formed here and stored at the end of the step
            if constexpr (NQ < NRS + 3) estage(std::integral_constant<int, NRS + 2>{}, y - 1, std::false_type{});
            estage(std::integral_constant<int, NRS + 3>{}, y - 1, std::true_type{});
          }
        } else if (y > yb) {
            uint32_t nxn = 0, nxo = 0;
#pragma unroll
            for (int q = 0; q < NCH; ++q) {
                const int c0 = CW * q;
                uint32_t sn[CW + 1], so[CW + 1], rn[CW], ro[CW];
                ref_chunk(par, c0, rn);
                ref_chunk(par + 1, c0, ro);
                s_chunk(par, c0, sn, nxn);
                s_chunk(par + 1, c0, so, nxo);
#pragma unroll
                for (int c = 0; c < CW; ++c) {
                    if (c0 + c < NC) {
                        if constexpr (ABS) {  // cs + |tn| - |to|: two v_sad_u16 (bytes) + one v_sub
                            cs[c0 + c] = __builtin_amdgcn_sad_u16(rn[c], sn[c], cs[c0 + c]) -
                                         __builtin_amdgcn_sad_u16(ro[c], so[c], 0u);
                        } else if constexpr (SSD) {  // u32 SSD (R > 5 or the right / volume passes)
                            const int tn = (int)rn[c] - (int)sn[c];
                            const int to = (int)ro[c] - (int)so[c];
                            const int nto = (int)so[c] - (int)ro[c];
                            // two v_mad_i32_i24 (cs + tn^2 + to * (-to)), not the 64-bit
                            // v_mad_u64_u32 that plain int products lowered to
                            cs[c0 + c] = (uint32_t)mad_i24(to, nto, mad_i24(tn, tn, (int)cs[c0 + c]));
                        } else {
                            // entering row into cs, leaving row summed apart and subtracted: each
                            // half of it is a term of that half of cs, so nothing borrows
                            const uint32_t en = sad_hi_u8(rn[c], pair_e1(sn, c), __builtin_amdgcn_sad_u8(rn[c], pair_e0(sn, c), as1(cs[c0 + c])));
                            const uint32_t lo = sad_hi_u8(ro[c], pair_e1(so, c), __builtin_amdgcn_sad_u8(ro[c], pair_e0(so, c), 0u));
                            cs[c0 + c] = as2(en - lo);
                        }
                    }
                }
            }
        }
        DSX_STAMP(1);
        DSX_STAMP(2);
        // ---- horizontal running box sum -> LDS tile (pixel k, disparity d0..) ----
        {
            uint8_t *tb = tile + d0 * CB;
            // Tile stores without an address VGPR (lds_store8_addtid): the pair layout outside the LR
            // pass, whose stores sit between the diagonal keys of single pixels.  The one-disparity
            // layouts keep ds_write_b32 (not measured with this form).
            constexpr bool ATID = kRowstepAtid && !SSD && SIDE != 3;
            auto abits = [](acc_t v) __attribute__((always_inline)) -> uint32_t {
                if constexpr (FSS) return __float_as_uint(v);
                else if constexpr (SSD) return v;
                else return as1(v);
            };
            acc_t acc = cs[0];
            if constexpr (FSS) acc = 8388608.0f + cs[0];  // + 2^23 (see FSS)
            if constexpr (!CG) {
#pragma unroll
            for (int c = 1; c <= 2 * R; ++c) {
                if constexpr (SSD) acc += cs[c];
                else acc = as2(as1(acc) + as1(cs[c]));
            }
            }
            if constexpr (side == 3) {
                // Right-view winners along the tile's diagonals: C_R(xr, d) = C(xr + m + d, d), so
                // right pixel xr collects keys (C << s | d) from (x, d) with x - m - d = xr.  Each
                // lane keeps the running key minimum of the diagonal through its slot(s); moving to
                // pixel k+1 a diagonal moves one disparity up (SAD: odd slot <- even slot, even slot
                // <- odd slot of lane-1; SSD: the slot of lane-1).  After the row every partial
                // minimum is combined across strips with a global atomicMin.  Keys of disparities
                // >= D (Dp padding) are forced to ~0 through the byte-permute selector (selector
                // byte 13 = 0xFF) / the d mask.
                //   SAD: the move is one v_min_u32_dpp wave_shr:1 (min_shr1: lane 0 keeps the new
                //        key) and the diagonal leaving the wave's top slot (lane 63) at pixel k is
                //        parked by that lane in the padding of tile row k (single-lane LDS store, no
                //        VALU); lanes 0..TX-2 pick the exits up after the row.  4 VALU per pixel
                //        for the two slots, against 7 for the register FIFO below.
                //   SSD: DPP wave_ror:1 hands the leaving diagonal to lane 0, from where a
                //        wave_shr:1 FIFO (E) collects it.  (The LDS exits measured slower here: the
                //        4-wave SSD pass is at its 128-VGPR budget and spilled more, C3 +9 %.)
                static_assert(SSD || NW <= 4, "SAD exit slots: 16 B of padding per tile row");
                const int ks = a.kshift;
                const uint32_t selE = d0 < D ? 0x05040100u : 0x0D0D0D0Du;
                const uint32_t selO = d0 + 1 < D ? 0x07060100u : 0x0D0D0D0Du;
                const uint32_t dmE = d0 < D ? (uint32_t)d0 : 0xFFFFFFFFu;
                const bool lane0 = ln == 0;
                const bool top = ln == 63;
                // SAD exits: pixel k's at xq + k * XST - a 128-B region per wave after the block's LDS
                // (the full-strip loop keeps 4 exits in registers and parks them with one single-lane
                // b128 store; r03: 31 exec-masked b32 stores per row cost ~6 % at C2r)
                constexpr bool XREG = !SSD;  // exits in the per-wave region
                uint8_t *xq = XREG ? smem + G::SMEM + G::XRB * wv : tile + Dp * CB + 4 * wv;
                constexpr int XST = XREG ? 4 : PITCH;
                uint32_t X[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
                uint32_t Ae = 0xFFFFFFFFu, Ao = 0xFFFFFFFFu, E = 0xFFFFFFFFu;
                // FULL: the strip lies inside the image and every lane owns real disparities
                // (D == Dp), so the per-pixel bounds / lane checks drop out of the unrolled loop
                auto diag_loop = [&](auto fullc) __attribute__((always_inline)) {
                    constexpr bool FULL = decltype(fullc)::value;
#pragma unroll
                    for (int k = 0; k < TX; ++k) {
                        if (k > 0) {
                            if constexpr (FSS) acc = (acc - cs[k - 1]) + cs[k + 2 * R];  // stays in [2^23, 2^24)
                            else if constexpr (SSD) acc = acc + cs[k + 2 * R] - cs[k - 1];
                            else acc = add_sub2(acc, cs[k + 2 * R], cs[k - 1]);
                        }
                        if (FULL || lane_writes) {
                            if constexpr (SSD) *reinterpret_cast<uint32_t *>(tb + k * PITCH) = abits(acc);
                            else *reinterpret_cast<uint32_t *>(tb + k * PITCH) = as1(acc);
                        }
                        if constexpr (SSD) {
                            if (FULL || x0 + k < W) Ae = umin2(Ae, (abits(acc) << ks) | dmE);
                            if (k < TX - 1) {
                                const uint32_t F = (uint32_t)__builtin_amdgcn_mov_dpp((int)Ae, 0x13C, 0xF, 0xF, false);  // wave_ror:1
                                E = (uint32_t)__builtin_amdgcn_update_dpp((int)F, (int)E, 0x138, 0xF, 0xF, false);  // wave_shr:1, lane 0 <- F
                                Ae = lane0 ? 0xFFFFFFFFu : F;
                            }
                        } else {
                            // (C << 16) | d by byte permute
                            const uint32_t kE = __builtin_amdgcn_perm(as1(acc), (uint32_t)d0, selE);
                            const uint32_t kO = __builtin_amdgcn_perm(as1(acc), (uint32_t)(d0 + 1), selO);
                            if constexpr (FULL) {
                                if (k > 0) {
                                    const uint32_t nE = min_shr1(Ao, kE);
                                    Ao = umin2(Ae, kO);
                                    Ae = nE;
                                } else {
                                    Ae = kE;
                                    Ao = kO;
                                }
                            } else {
                                if (k > 0) {  // one disparity up: wave_shr:1, lane 0 <- ~0
                                    const uint32_t sh = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)Ao, 0x138, 0xF, 0xF, false);
                                    Ao = Ae;
                                    Ae = sh;
                                }
                                if (x0 + k < W) {
                                    Ae = umin2(Ae, kE);
                                    Ao = umin2(Ao, kO);
                                }
                            }
                            if (k < TX - 1) {  // exit
                                if constexpr (FULL) {
                                    X[k & 3] = Ao;
                                    if (((k & 3) == 3 || k == TX - 2) && top)
                                        *reinterpret_cast<uint4 *>(xq + (k & ~3) * 4) = make_uint4(X[0], X[1], X[2], X[3]);
                                } else if (top) {
                                    *reinterpret_cast<uint32_t *>(xq + k * XST) = Ao;
                                }
                            }
                        }
                    }
                };
                // chosen per segment (template): with both forms in one row loop, hipcc hoisted the
                // 31 per-pixel bounds of the partial form out of the loop as 62 SGPRs, which spilled
                // through v_writelane / v_readlane in every row step of every strip
                if constexpr (LRFULL) diag_loop(std::true_type{});
                else diag_loop(std::false_type{});
                uint32_t *krow = a.lr_keys + fout + (long)y * W;
                const int dtop = (wv + 1) * G::LDW - 1;  // disparity of the wave's top slot
                if constexpr (SSD) {
                    const int xe = x0 + (TX - 2 - ln) - m - dtop;  // E lane j: exit of pixel TX-2-j
                    if (ln < TX - 1 && E != 0xFFFFFFFFu && xe >= 0 && xe < W) atomicMin(krow + xe, E);
                } else if (ln < TX - 1) {
                    E = *reinterpret_cast<const uint32_t *>(xq + ln * XST);  // exit of pixel ln, parked in LDS
                    const int xe = x0 + ln - m - dtop;
                    if (E != 0xFFFFFFFFu && xe >= 0 && xe < W) atomicMin(krow + xe, E);
                }
                const int xa = x0 + TX - 1 - m - d0;
                if (Ae != 0xFFFFFFFFu && xa >= 0 && xa < W) atomicMin(krow + xa, Ae);
                if constexpr (!SSD) {
                    if (Ao != 0xFFFFFFFFu && xa - 1 >= 0 && xa - 1 < W) atomicMin(krow + xa - 1, Ao);
                }
            } else if (ATID && lane_writes) {
                // lane-indexed stores, eight pixels per statement: tb = tile + wv * LDW * CB + 4 * lane
                static_assert(!ATID || (TX % 8 == 0 && G::LDW * CB == 256), "addtid: a lane's tile bytes are 4 * lane");
                if constexpr (ATID) {
                const uint32_t mb = lds_offset(tile) + (uint32_t)wvu * (uint32_t)(G::LDW * CB);
                auto grp = [&](auto k0c) __attribute__((always_inline)) {
                    constexpr int k0 = decltype(k0c)::value;
                    uint32_t v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if constexpr (CG) {  // three group sums (R = 4) or one (R = 1): independent, no running sum
                            v[j] = R == 4 ? add3_u32(as1(cs[k0 + j]), as1(cs[k0 + j + 3]), as1(cs[k0 + j + 6])) : as1(cs[k0 + j]);
                        } else {
                            if (k0 + j > 0) acc = add_sub2(acc, cs[k0 + j + 2 * R], cs[k0 + j - 1]);
                            v[j] = as1(acc);
                        }
                    }
                    lds_store8_addtid<k0 * PITCH, PITCH>(mb, v);
                };
                grp(std::integral_constant<int, 0>{});
                grp(std::integral_constant<int, 8>{});
                grp(std::integral_constant<int, 16>{});
                grp(std::integral_constant<int, 24>{});
                }
            } else if (lane_writes) {
#pragma unroll
                for (int k = 0; k < TX; ++k) {
                    if (k > 0) {
                        if constexpr (FSS) acc = (acc - cs[k - 1]) + cs[k + 2 * R];
                        else if constexpr (SSD) acc = acc + cs[k + 2 * R] - cs[k - 1];
                        else acc = add_sub2(acc, cs[k + 2 * R], cs[k - 1]);
                    }
                    if constexpr (SSD) *reinterpret_cast<uint32_t *>(tb + k * PITCH) = abits(acc);
                    else *reinterpret_cast<uint32_t *>(tb + k * PITCH) = as1(acc);
                }
            }
            if (dodd && d0 + 1 == D) {  // odd D: the high half of the last pair is disparity D
                for (int k = 0; k < TX; ++k) *reinterpret_cast<uint16_t *>(tb + k * PITCH + 2) = (uint16_t)padv;
            }
            if (edge && lane_writes) {  // right pass: x + m + d must stay inside [0, W-1]
                const int base = x0 + m + d0;
                for (int k = 0; k < TX; ++k) {
                    const int p0 = base + k;
                    if constexpr (SSD) {
                        if (p0 < 0 || p0 > W - 1) *reinterpret_cast<uint32_t *>(tb + k * PITCH) = padv;
                    } else {
                        if (p0 < 0 || p0 > W - 1) *reinterpret_cast<uint16_t *>(tb + k * PITCH) = (uint16_t)padv;
                        if (p0 + 1 < 0 || p0 + 1 > W - 1) *reinterpret_cast<uint16_t *>(tb + k * PITCH + 2) = (uint16_t)padv;
                    }
                }
            }
        }
        DSX_STAMP(3);
        // the lane-indexed tile stores are invisible to the compiler's lgkmcnt bookkeeping: drained
        // by hand before the barrier that publishes the tile to the block's other waves
        if constexpr (kRowstepAtid && !SSD && SIDE != 3 && NW > 1) lds_drain();
        block_sync<NW>();
        DSX_STAMP(4);
        // The prefetched rows go to LDS here, before the epilogue's output stores: the loads have
        // had the column update and the box phase to land, and no store is younger than them, so
        // the waits below never drain a store (after the epilogue they came out as vmcnt(1) / (0)
        // behind the step's two stores, a full store round trip per row).  Safe: slots par ^ 2 and
        // (par ^ 2) + 1 were last read by the column update of step y - 1, every wave of the
        // block has passed the mid-step barrier above since then, and the barrier that ends the
        // step orders these writes before step y + 1 reads them (the end barrier of step y - 1 alone
        // already separates them from their last readers).  The epilogue reads the tile only.
        // That holds for the sequential loops.  Rotated (OVL), the step's stores are those of row y - 1's tail, whose
        // outputs were formed behind the last chunk: they follow the staging (estore below).
        if constexpr (RL2) {
            // the lane's staging address alternates between slots 0 and 2: carried across the steps and
            // flipped with one subtraction (rebuilt from par, it came out as one v_mad per store)
            if constexpr (MRG) {
                if (more) {
                    stm(smem + stg, pn0);
                    stm(smem + stg + SLOT, po0);
                }
                stg = (2 * m_lane + (uint32_t)(2 * SLOT)) - stg;
            } else if constexpr (SIDE != 3) {
                if (more) {
                    st_at(smem + stg, pn0, pn1, pn2, pn3, pnr);
                    st_at(smem + stg + SLOT, po0, po1, po2, po3, por);
                }
                stg = (uint32_t)(32 * tid + 2 * SLOT) - stg;
            } else if (more) {  // LR pass, at its register budget: no carried address (R = 1 spilled 16 B more)
                st(par ^ 2, pn0, pn1, pn2, pn3, pnr);
                st((par ^ 2) + 1, po0, po1, po2, po3, por);
            }
        }
        if constexpr (OVL) {  // row y - 1's outputs, formed behind the last chunk
            if (y > yb) estore(y - 1, a);
        }
        DSX_STAMP(5);
        if constexpr (side == 2) {
            // ---- cost volume store: TX pixels x Dp costs, 16-B chunks ----
            constexpr int CPP = Dp * CB / 16;
            for (int q = tid; q < TX * CPP; q += NT) {
                const int k = q / CPP, off = (q - k * CPP) * 16;
                const int x = x0 + k;
                if (x < W) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(tile + k * PITCH + off);
                    *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(a.vol) + ((size_t)fout + (size_t)y * W + x) * (Dp * CB) + off) = v;
                }
            }
        } else if constexpr (!OVL) {
            // ---- epilogue: TPP lanes per pixel ----
            const int k = tid / TPP, h = tid % TPP;
            const int x = x0 + k;
            const uint8_t *px = tile + k * PITCH + h * DSL * CB;
            uint32_t bs[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                if constexpr (SSD) {
                    const uint4 v0 = *reinterpret_cast<const uint4 *>(px + 32 * i);
                    const uint4 v1 = *reinterpret_cast<const uint4 *>(px + 32 * i + 16);
                    bs[i] = umin2(umin2(umin2(v0.x, v0.y), umin2(v0.z, v0.w)), umin2(umin2(v1.x, v1.y), umin2(v1.z, v1.w))) - OFF;
                } else {
                    const uint4 v = *reinterpret_cast<const uint4 *>(px + 16 * i);
                    const u16x2 mm = __builtin_elementwise_min(__builtin_elementwise_min(as2(v.x), as2(v.y)),
                                                               __builtin_elementwise_min(as2(v.z), as2(v.w)));
                    bs[i] = umin2(mm.x, mm.y);
                }
            }
            // Two argmin forms, chosen per instantiation from measurements (r01e): the key tree
            // wins on the LR pass (C3, C4) and 15x15 windows (C5); the compare/select scan keeps
            // the SIDE 0 pass at <= 11x11 at 151 VGPRs (the key tree costs C2 +7 %).  That scan is
            // what the one-disparity layouts still take there; the pair layout has its own, cheaper
            // keys (KEY2 below: C2 54.5 -> 53.8 us against the scan).
            constexpr bool KEYS = SIDE == 3 || R >= 6;
            constexpr bool KEY2 = kRowstepKey2 && !KEYS && !SSD;
            uint32_t cb, dl;
            if constexpr (KEYS) {
                // lowest-d argmin without compare/select scans: keys (cost << GB | global block) give
                // the minimum and its lowest block in one min tree; the owning lane then keys the 8
                // costs of that block (cost << 3 | e).  Costs < 2^24 (SSD) / 2^16 (SAD), GB <= 6.
                constexpr int GB = Dp / 8 <= 16 ? 4 : (Dp / 8 <= 32 ? 5 : 6);
                uint32_t kmin = 0xFFFFFFFFu;
    #pragma unroll
                for (int i = 0; i < NB; ++i) kmin = umin2(kmin, (bs[i] << GB) | (uint32_t)(h * NB + i));
                kmin = gmin<TPP>(kmin);
                cb = kmin >> GB;
                const int gblk = (int)(kmin & ((1u << GB) - 1u));
                dl = 0xFFFFu;
                if (gblk / NB == h) {
                    const int bsel = gblk - h * NB;
                    uint32_t k8 = 0xFFFFFFFFu;
                    if constexpr (SSD) {
                        const uint4 v0 = *reinterpret_cast<const uint4 *>(px + 32 * bsel);
                        const uint4 v1 = *reinterpret_cast<const uint4 *>(px + 32 * bsel + 16);
                        const uint32_t c8[8] = {v0.x - OFF, v0.y - OFF, v0.z - OFF, v0.w - OFF,
                                                v1.x - OFF, v1.y - OFF, v1.z - OFF, v1.w - OFF};
    #pragma unroll
                        for (int q = 0; q < 8; ++q) k8 = umin2(k8, (c8[q] << 3) | (uint32_t)q);
                    } else {
                        const uint4 v = *reinterpret_cast<const uint4 *>(px + 16 * bsel);
                        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    #pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            k8 = umin2(k8, ((w4[q] & 0xFFFFu) << 3) | (uint32_t)(2 * q));
                            k8 = umin2(k8, ((w4[q] >> 16) << 3) | (uint32_t)(2 * q + 1));
                        }
                    }
                    dl = (uint32_t)(h * DSL + 8 * bsel + (int)(k8 & 7u));
                }
            } else if constexpr (KEY2) {
                // Keys again, in the cheapest form for the packed u16 costs: the block key is one
                // v_lshl_or_b32 with an inline block index (the lane's h * NB is or-ed in once, after the
                // lane's own minimum: it is common to the lane's keys and its bits are clear in them), and
                // an element key keeps the cost where it lies - low halves shifted up 16 (v_lshl_or_b32),
                // high halves masked in place (v_and_or_b32) - with the element index in the low bits.
                // Every lane keys the block of that index in its own slice (no branch); only the owner's
                // result counts.  12 + 12 VALU against 20 + 22 with 15 s_nop for the scans below.
                static_assert((NB & (NB - 1)) == 0, "block index bits");
                constexpr int GB = Dp / 8 <= 16 ? 4 : (Dp / 8 <= 32 ? 5 : 6);
                uint32_t kmin = 0xFFFFFFFFu;
    #pragma unroll
                for (int i = 0; i < NB; ++i) kmin = umin2(kmin, (bs[i] << GB) | (uint32_t)i);
                kmin = gmin<TPP>(kmin | (uint32_t)(h * NB));
                cb = kmin >> GB;
                const uint32_t gblk = kmin & ((1u << GB) - 1u);
                const uint4 v = *reinterpret_cast<const uint4 *>(px + 16 * (gblk & (NB - 1)));
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
                uint32_t k8 = 0xFFFFFFFFu;
    #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    k8 = umin2(k8, (w4[q] << 16) | (uint32_t)(2 * q));
                    k8 = umin2(k8, (w4[q] & 0xFFFF0000u) | (uint32_t)(2 * q + 1));
                }
                dl = (int)(gblk / NB) == h ? gblk * 8 + (k8 & 7u) : 0xFFFFu;
            } else {
                uint32_t lmin = bs[0];
    #pragma unroll
                for (int i = 1; i < NB; ++i) lmin = umin2(lmin, bs[i]);
                cb = gmin<TPP>(lmin);
                int bsel = -1;
    #pragma unroll
                for (int i = NB - 1; i >= 0; --i) bsel = bs[i] == cb ? i : bsel;
                dl = 0xFFFFu;
                if (bsel >= 0) {
                    uint32_t c8[8];
                    if constexpr (SSD) {
                        const uint4 v0 = *reinterpret_cast<const uint4 *>(px + 32 * bsel);
                        const uint4 v1 = *reinterpret_cast<const uint4 *>(px + 32 * bsel + 16);
                        c8[0] = v0.x - OFF; c8[1] = v0.y - OFF; c8[2] = v0.z - OFF; c8[3] = v0.w - OFF;
                        c8[4] = v1.x - OFF; c8[5] = v1.y - OFF; c8[6] = v1.z - OFF; c8[7] = v1.w - OFF;
                    } else {
                        const uint4 v = *reinterpret_cast<const uint4 *>(px + 16 * bsel);
                        c8[0] = v.x & 0xFFFFu; c8[1] = v.x >> 16; c8[2] = v.y & 0xFFFFu; c8[3] = v.y >> 16;
                        c8[4] = v.z & 0xFFFFu; c8[5] = v.z >> 16; c8[6] = v.w & 0xFFFFu; c8[7] = v.w >> 16;
                    }
                    int e = 7;
    #pragma unroll
                    for (int q = 6; q >= 0; --q) e = c8[q] == cb ? q : e;
                    dl = (uint32_t)(h * DSL + 8 * bsel + e);
                }
            }
            const int b = (int)gmin<TPP>(dl);
            const long o = fout + (long)y * W + x;
            if constexpr (side == 1) {
                if (h == 0 && x < W) a.out_dR[o] = cb == padv ? (int16_t)-1 : (int16_t)b;
            } else {
                // valid band: A5' [m + D - 1, W - 1 + m]; OpenCV's form (sg_keys) [max(m + D, 0), W + min(m, 0))
                bool valid = SGK ? (x < W && x >= max(m + D, 0) && x < W + min(m, 0))
                                       : (x < W && x >= m + D - 1 && x <= W - 1 + m);
                if (a.uniq > 0) {
                    const int rel = b - h * DSL;
                    uint32_t nm = 0xFFFFFFFFu;
#pragma unroll
                    for (int i = 0; i < NB; ++i) {
                        const bool hit = rel >= 8 * i - 1 && rel <= 8 * i + 8;
                        nm = hit ? nm : umin2(nm, bs[i]);
                    }
                    const int ib0 = (rel - 1) >> 3, ib1 = (rel + 1) >> 3;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int ib = t == 0 ? ib0 : ib1;
                        if (ib >= 0 && ib < NB && (t == 0 || ib1 != ib0)) {
                            // one wide read of the block, selects instead of per-element branches
                            uint32_t c8[8];
                            if constexpr (SSD) {
                                const uint4 v0 = *reinterpret_cast<const uint4 *>(px + 32 * ib);
                                const uint4 v1 = *reinterpret_cast<const uint4 *>(px + 32 * ib + 16);
                                c8[0] = v0.x - OFF; c8[1] = v0.y - OFF; c8[2] = v0.z - OFF; c8[3] = v0.w - OFF;
                                c8[4] = v1.x - OFF; c8[5] = v1.y - OFF; c8[6] = v1.z - OFF; c8[7] = v1.w - OFF;
                            } else {
                                const uint4 v = *reinterpret_cast<const uint4 *>(px + 16 * ib);
                                c8[0] = v.x & 0xFFFFu; c8[1] = v.x >> 16; c8[2] = v.y & 0xFFFFu; c8[3] = v.y >> 16;
                                c8[4] = v.z & 0xFFFFu; c8[5] = v.z >> 16; c8[6] = v.w & 0xFFFFu; c8[7] = v.w >> 16;
                            }
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const int dd = 8 * ib + e - rel;
                                nm = (dd > 1 || dd < -1) ? umin2(nm, c8[e]) : nm;
                            }
                        }
                    }
                    nm = gmin<TPP>(nm);
                    // real costs are < min(padv, 2^24) (SSD 15x15 max 14.6M); a larger minimum is
                    // padding only, i.e. no competitor (the oracle's "no far d"), and the products
                    // then fit 32 bits
                    const uint32_t real_max = padv < (1u << 24) ? padv : (1u << 24);
                    if (nm < real_max && nm * (uint32_t)(100 - a.uniq) < cb * 100u) valid = false;
                }
                int32_t f = b * 16;
                float pf = (float)(m + b);
                if (a.subpix && b > 0 && b < D - 1) {
                    int32_t cm, cp;
                    const uint8_t *pk = tile + k * PITCH;
                    if constexpr (SSD) {
                        cm = (int32_t)(reinterpret_cast<const uint32_t *>(pk)[b - 1] - OFF);
                        cp = (int32_t)(reinterpret_cast<const uint32_t *>(pk)[b + 1] - OFF);
                    } else {
                        cm = reinterpret_cast<const uint16_t *>(pk)[b - 1];
                        cp = reinterpret_cast<const uint16_t *>(pk)[b + 1];
                    }
                    int32_t den = cm + cp - 2 * (int32_t)cb;
                    den = den < 1 ? 1 : den;
                    if constexpr (DIVQ) f += subpix_quot((cm - cp) * 16 + den, 2 * den);
                    else f += div_trunc_small((cm - cp) * 16 + den, 2 * den);
                    if (a.float_mode == 1) pf = (float)(m + b) + (float)(cm - cp) / (float)(2 * den);
                }
                if (h == 0 && x < W) {
                    if (lr_on) a.dstar[o] = valid ? (int16_t)b : (int16_t)-1;  // LR check: lr_fixup
                    const int16_t fx = valid ? (int16_t)(m * 16 + f) : (int16_t)((m - 1) * 16);
                    if constexpr (SGK) {
                        // OpenCV's LR form: a unique winner offers (cost, d) to right pixel x - m - d
                        // (min cost, then max d); lr_fixup_sgbm tests against them afterwards
                        a.dstar[o] = fx;
                        if (valid)
                            atomicMin(a.sg_keys + fout + (long)y * W + (x - m - b),
                                      (cb << a.kshift) | (((1u << a.kshift) - 1u) - (uint32_t)b));
                    }
                    if (a.out_fixed) a.out_fixed[o] = fx;
                    if (a.out_float) a.out_float[o] = a.float_mode == 0 ? (float)fx * 0.0625f : (valid ? pf : (float)(m - 1));
                }
            }
        }
        if (!RL2 && more) {  // first form: staged behind the epilogue
            st(par ^ 2, pn0, pn1, pn2, pn3, pnr);
            st((par ^ 2) + 1, po0, po1, po2, po3, por);
        }
        DSX_STAMP(6);
        block_sync<NW>();
        DSX_STAMP(7);
    }
    if constexpr (OVL) {  // the segment's last row: nothing is kept across segments
        auto dr = [&](auto sc) __attribute__((always_inline)) {
            if constexpr (decltype(sc)::value <= NRS + 3) estage(sc, ye - 1, std::false_type{});
        };
        dr(std::integral_constant<int, 0>{}); dr(std::integral_constant<int, 1>{}); dr(std::integral_constant<int, 2>{});
        dr(std::integral_constant<int, 3>{}); dr(std::integral_constant<int, 4>{}); dr(std::integral_constant<int, 5>{});
        dr(std::integral_constant<int, 6>{}); dr(std::integral_constant<int, 7>{}); dr(std::integral_constant<int, 8>{});
        dr(std::integral_constant<int, 9>{}); dr(std::integral_constant<int, 10>{}); dr(std::integral_constant<int, 11>{});
    }
}

template <int R, bool SSD, int NW, int SIDE, bool ABS>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu((SSD && NW >= 4) ? kWpeSsd : kWpe))) void bm2(Bm2Args a) {
    using G = Geo<R, SSD, NW>;
    constexpr int TX = G::TX, NT = G::NT, NC = G::NC, NJ = G::NJ;
    constexpr int side = SIDE;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int wvu = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.H, W = a.W, m = a.m;
    // block timeline: the start stamp goes out at once (nothing held live across the segments)
    if (a.timeline && wvu == 0 && __lane_id() == 0) a.timeline[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#ifdef DSX_STAMPS
    uint64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t_prev = 0;
    uint64_t nsteps = 0;
#endif

    // ---- left pass: columns of strips that lie entirely in the invalid band ----
    if ((side == 0 || side == 3 || side == 4) && (a.out_fixed || a.out_float)) {
        const int xa = a.strip_begin * TX, xb = min(W, (a.strip_begin + a.strip_count) * TX);
        const int nin = xa + (W - xb);
        const int total = nin * H * a.nframes;  // frames are H-row slabs of one tall output (< 2^31)
        const int16_t fi = (int16_t)((m - 1) * 16);
        for (int q = blockIdx.x * NT + tid; q < total; q += gridDim.x * NT) {
            const int y = q / nin;
            const int c = q - y * nin;
            const int x = c < xa ? c : xb + (c - xa);
            const long o = (long)y * W + x;
            if (a.out_fixed) a.out_fixed[o] = fi;
            if (a.out_float) a.out_float[o] = (float)(m - 1);
            if constexpr (side == 4) a.dstar[o] = fi;  // lr_fixup_sgbm reads every pixel
        }
    }

    // ---- LR pass: reset the other key half (the previous call's keys, already checked) ----
    if ((side == 3 || side == 4) && a.lr_reset_n > 0) {
        uint32_t *kr = a.lr_reset;
        const int64_t n = a.lr_reset_n, stride = (int64_t)gridDim.x * NT;
        const int64_t t0 = (int64_t)blockIdx.x * NT + tid;
        if (((uintptr_t)kr & 15u) == 0) {
            for (int64_t q = t0; q < n / 4; q += stride)
                reinterpret_cast<uint4 *>(kr)[q] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            for (int64_t q = n / 4 * 4 + t0; q < n; q += stride) kr[q] = 0xFFFFFFFFu;
        } else {
            for (int64_t q = t0; q < n; q += stride) kr[q] = 0xFFFFFFFFu;
        }
    }

    // ---- work partition (host-computed, bm2_partition): block b owns linear (frame, strip, row)
    // units [part[b], part[b+1]); nframes * H * W < 2^31 (host check)
    const int lin0 = a.part[blockIdx.x], lin1 = a.part[blockIdx.x + 1];
    constexpr bool lr_on = SIDE == 3;  // left pass that also builds the right-view winners
    int qcur = -1;
    int pe[3];  // rows done at which the priority drops (progress bands pt1..pt3 of 256)
    {
        const int tot = lin1 - lin0;
        pe[0] = (a.pt1 * tot + 255) >> 8;
        pe[1] = (a.pt2 * tot + 255) >> 8;
        pe[2] = (a.pt3 * tot + 255) >> 8;
    }
    for (int it = lin0; it < lin1;) {
        const int sidx = it / H;
        const int f = sidx / a.strip_count;
        const int s = a.strip_begin + (sidx - f * a.strip_count);
        const long fin = (long)f * a.frame_stride, fout = (long)f * H * W;
        const int yb = it - sidx * H;
        const int ye = min(H, yb + (lin1 - it));
        const int done0 = it - lin0;
        it += ye - yb;
        const int x0 = s * TX;
        // bm2_fast (dsx_partition.h) is this expression; a call to it compiles to other code, so it is written out
        const int PB = side == 1 ? (x0 - R + m) : (x0 - R - m + NC - 1);
        const int NJ4 = (NJ + 3) / 4;
        const bool fast = (side == 1 ? (PB >= 0 && PB + 4 * NJ4 <= W - 1) : (PB - 4 * NJ4 >= 0 && PB <= W - 1)) &&
                          x0 - R >= 0 && x0 - R + 4 * ((NC + 3) / 4) - 1 <= W - 1;
#ifdef DSX_STAMPS
#define DSX_SEG(FASTV, FULLV) \
    bm2_segment<R, SSD, NW, SIDE, FASTV, ABS, FULLV>(a, smem, x0, yb, ye, fin, fout, lr_on, done0, pe, qcur, wvu, ph, t_prev, nsteps)
#else
#define DSX_SEG(FASTV, FULLV) bm2_segment<R, SSD, NW, SIDE, FASTV, ABS, FULLV>(a, smem, x0, yb, ye, fin, fout, lr_on, done0, pe, qcur, wvu)
#endif
        // LR pass: strips inside the image with D == Dp take the check-free diagonal loop
        const bool lrfull = side == 3 && x0 + TX <= W && a.D == G::Dp;
        if (fast) {
            if (lrfull) DSX_SEG(true, true);
            else DSX_SEG(true, false);
        } else {
            if (lrfull) DSX_SEG(false, true);
            else DSX_SEG(false, false);
        }
#undef DSX_SEG
    }
    if (a.timeline && wvu == 0 && __lane_id() == 0) {
        const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
        uint64_t *tl = a.timeline + 4 * blockIdx.x;
        tl[1] = t_end;
        tl[2] = (uint64_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_REG_HW_ID
        tl[3] = (uint64_t)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (15 << 11));  // HW_REG_XCC_ID
#ifdef DSX_STAMPS
        uint64_t *ps = a.timeline + 4 * 65536 + 8 * blockIdx.x;
        for (int i = 0; i < 7; ++i) ps[i] = ph[i];
        ps[7] = nsteps;
#endif
    }
}


// Device copies of partitions, one per launch shape (a launch in flight on any stream may still
// read one, so entries are only dropped after a device-wide drain, at 256 shapes).  The caller
// holds launch_mutex() from the lookup through the kernel launch: a table handed out is enqueued
// on its stream before any other thread can evict (and so drain before freeing) it.
struct PartKey {
    int dev, NG, S, sb, nframes, H, XL, XU, w8, nlev, w[4];
    bool operator==(const PartKey &o) const { return memcmp(this, &o, sizeof(PartKey)) == 0; }
};
static std::mutex &launch_mutex() {
    static std::mutex mu;  // shared by every bm2 instantiation of this translation unit
    return mu;
}
static hipError_t bm2_partition_dev(const PartKey &k, int TX, const int **out) {
    static std::vector<std::pair<PartKey, int *>> cache;
    for (const auto &e : cache)
        if (e.first == k) {
            *out = e.second;
            return hipSuccess;
        }
    if (cache.size() >= 256) {
        // bounded: drain every device that holds a table, then drop them all (a process cycling
        // through many shapes pays one synchronisation per 256 new shapes)
        int prev = 0;
        (void)hipGetDevice(&prev);
        for (size_t i = 0; i < cache.size(); ++i) {
            bool seen = false;
            for (size_t j = 0; j < i; ++j) seen = seen || cache[j].first.dev == cache[i].first.dev;
            if (seen) continue;
            (void)hipSetDevice(cache[i].first.dev);
            hipError_t se = hipDeviceSynchronize();
            if (se != hipSuccess) {
                (void)hipSetDevice(prev);
                return se;
            }
        }
        for (auto &e : cache) {
            (void)hipSetDevice(e.first.dev);
            (void)hipFree(e.second);
        }
        (void)hipSetDevice(prev);
        cache.clear();
    }
    const std::vector<int> part = bm2_partition(k.NG, k.S, k.sb, k.nframes, k.H, k.XL, k.XU, TX, k.w8, k.nlev, k.w);
    int *d = nullptr;
    hipError_t e = hipMalloc(&d, part.size() * sizeof(int));
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, part.data(), part.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return e;
    }
    cache.emplace_back(k, d);
    *out = d;
    return hipSuccess;
}

template <int R, bool SSD, int NW, int SIDE, bool ABS = false>
static hipError_t launch_bm2_side(const Bm2Args &a, hipStream_t st) {
    using G = Geo<R, SSD, NW>;
    // + the LR exit region; the LDS-diagonal SSD LR pass reads up to TX * 4 - 24 B past the tile
    constexpr int SM = G::SMEM + ((SIDE == 3 && !SSD) ? G::XRB * NW : 0);
    const void *fn = (const void *)bm2<R, SSD, NW, SIDE, ABS>;
    static int blocks_per_cu[64] = {};
    static int num_cu[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    // serialises the first-launch occupancy query per device and the partition-table lookup
    // through the launch itself (see bm2_partition_dev)
    std::lock_guard<std::mutex> lock(launch_mutex());
    if (!blocks_per_cu[dev]) {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, SM);
        if (e != hipSuccess) return e;
        int nb = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, G::NT, SM);
        if (e != hipSuccess) return e;
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        // the residency bm2_grid plans with; DSX_BLOCKS_PER_CU_ADJ (e.g. -1) adjusts it for tuning
        const char *adj = getenv("DSX_BLOCKS_PER_CU_ADJ");
        const int nbr = nb + (adj ? atoi(adj) : 0);
        blocks_per_cu[dev] = nbr > 1 ? nbr : 1;
        num_cu[dev] = cus > 0 ? cus : 1;
    }
    // the switches of bm2_grid's two reduced-grid rules: DSX_SMALL_GRID=0 / DSX_FLIGHT_GRID=0 disable one
    static const bool small_grid = [] {
        const char *e = getenv("DSX_SMALL_GRID");
        return !(e && *e == '0');
    }();
    static const bool flight_grid = [] {
        const char *e = getenv("DSX_FLIGHT_GRID");
        return !(e && *e == '0');
    }();
    const Bm2Grid plan = bm2_grid(blocks_per_cu[dev], num_cu[dev], R, NW, SSD, SIDE, ABS, (long)a.strip_count * a.nframes * a.H,
                                  a.nframes, a.in_flight != 0, a.grid_override, small_grid, flight_grid);
    const long grid = plan.grid;
    static const bool verbose = getenv("DSX_VERBOSE") != nullptr;  // diagnostics: read once
    if (verbose)
        fprintf(stderr, "[dsx] bm2<R=%d,SSD=%d,NW=%d,SIDE=%d> grid %ld (%d/CU) smem %d\n", R, (int)SSD, NW, SIDE, grid,
                blocks_per_cu[dev], SM);
    // the float block minima take finite f16 patterns: a host built without the switch would pad with a NaN pattern
    if (bm2_blockmin(R, SSD ? BM_SSD : (ABS ? BM_SAD1 : BM_SAD), NW, SIDE, false) && a.padv > kBlockminPad) return hipErrorInvalidValue;
    Bm2Args la = a;
    la.nlev = plan.nlev;
    {
        const Bm2Interval fi = bm2_fast_interval(SIDE, R, G::NC, G::NJ, a.W, a.m);
        PartKey k;
        memset(&k, 0, sizeof(k));
        k.dev = dev, k.NG = (int)grid, k.S = a.strip_count, k.sb = a.strip_begin, k.nframes = a.nframes, k.H = a.H;
        k.XL = fi.XL, k.XU = fi.XU, k.w8 = a.slow_w8, k.nlev = la.nlev;
        for (int i = 0; i < 4; ++i) k.w[i] = la.nlev > 1 ? a.agew[i] : 64;
        e = bm2_partition_dev(k, G::TX, &la.part);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((bm2<R, SSD, NW, SIDE, ABS>), dim3((unsigned)grid), dim3(G::NT), SM, st, la);
    return hipGetLastError();
}

template <int R, bool SSD, int NW>
static hipError_t launch_bm2_one(const Bm2Args &a, hipStream_t st) {
    switch (a.side) {
        // the OpenCV-form keys are a separate build of the left pass: kept out of the plain one
        // (their runtime branches cost the C2 pass 2 %, profiles/r04n_sg_side0_ab.txt)
        case 0: return a.sg_keys ? launch_bm2_side<R, SSD, NW, 4>(a, st) : launch_bm2_side<R, SSD, NW, 0>(a, st);
        case 1: return launch_bm2_side<R, SSD, NW, 1>(a, st);
        case 3: return launch_bm2_side<R, SSD, NW, 3>(a, st);
        default: return launch_bm2_side<R, SSD, NW, 2>(a, st);
    }
}

// SAD1 (kind BM_SAD1): fused left / right passes only (pick_geometry never selects it for the volume)
template <int R>
static hipError_t launch_bm2_sad1(const Bm2Args &a, hipStream_t st) {
    switch (a.side) {
        case 0: return a.sg_keys ? launch_bm2_side<R, true, 1, 4, true>(a, st) : launch_bm2_side<R, true, 1, 0, true>(a, st);
        case 1: return launch_bm2_side<R, true, 1, 1, true>(a, st);
        case 3: return launch_bm2_side<R, true, 1, 3, true>(a, st);
        default: return hipErrorInvalidValue;
    }
}

template <int R>
static hipError_t launch_bm2_r(int kind, int nw, const Bm2Args &a, hipStream_t st) {
    if (kind == BM_SAD1) return nw == 1 ? launch_bm2_sad1<R>(a, st) : hipErrorInvalidValue;
    if (kind == BM_SAD) {
        switch (nw) {
            case 1: return launch_bm2_one<R, false, 1>(a, st);
            case 2: return launch_bm2_one<R, false, 2>(a, st);
            case 4: return launch_bm2_one<R, false, 4>(a, st);
        }
    } else {
        switch (nw) {
            case 1: return launch_bm2_one<R, true, 1>(a, st);
            case 2: return launch_bm2_one<R, true, 2>(a, st);
            case 4: return launch_bm2_one<R, true, 4>(a, st);
            case 8: return launch_bm2_one<R, true, 8>(a, st);
        }
    }
    return hipErrorInvalidValue;
}

#define DSX_DECL_BM2(r) hipError_t launch_bm2_radius_##r(int, int, const Bm2Args &, hipStream_t);
DSX_DECL_BM2(0) DSX_DECL_BM2(1) DSX_DECL_BM2(2) DSX_DECL_BM2(3)
DSX_DECL_BM2(4) DSX_DECL_BM2(5) DSX_DECL_BM2(6) DSX_DECL_BM2(7)

#ifdef DSX_RADIUS
#define DSX_CAT2(x, y) x##y
#define DSX_CAT(x, y) DSX_CAT2(x, y)
hipError_t DSX_CAT(launch_bm2_radius_, DSX_RADIUS)(int kind, int nw, const Bm2Args &a, hipStream_t st) {
    return launch_bm2_r<DSX_RADIUS>(kind, nw, a, st);
}
#else
hipError_t launch_bm2(int radius, int kind, int nw, const Bm2Args &a, hipStream_t st) {
    switch (radius) {
        case 0: return launch_bm2_radius_0(kind, nw, a, st);
        case 1: return launch_bm2_radius_1(kind, nw, a, st);
        case 2: return launch_bm2_radius_2(kind, nw, a, st);
        case 3: return launch_bm2_radius_3(kind, nw, a, st);
        case 4: return launch_bm2_radius_4(kind, nw, a, st);
        case 5: return launch_bm2_radius_5(kind, nw, a, st);
        case 6: return launch_bm2_radius_6(kind, nw, a, st);
        case 7: return launch_bm2_radius_7(kind, nw, a, st);
        default: return hipErrorInvalidValue;
    }
}
#endif

}  // namespace dsx
