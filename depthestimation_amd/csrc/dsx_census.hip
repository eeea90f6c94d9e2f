// Census block costs (dsx_params.cost = DSX_COST_CENSUS9X7 / DSX_COST_CENSUS5X5): the Hamming distance
// between census codes, summed over this build's A5' block window.  An addition of this build (as the
// matcher prefilter is): parity with nothing outside this repository is claimed.  The arithmetic is
// depthestimation_amd/census.py's; the volume has K1's layout ([H][W][Dp] u16, pads >= D), so K2
// (uniqueness, sub-pixel, LR) and the SGM passes run on it unchanged.
//
// Two launches, both streaming:
//   census_transform : the code T(I)(x, y) of every pixel of both views (grid z = view).  Neighbours in
//             row-major order, the centre skipped, bit k = I(neighbour k) < I(centre); 62 bits (9x7,
//             8-B codes) or 24 bits (5x5, 4-B codes inside the handle, 8-B from dsx_census_device).
//   census_volume    : block costs straight into the volume, one pass.  One wave owns 128 disparities
//             (lane l the pair (2l, 2l+1), two u16 in one VGPR), a strip of kCvTX columns and a segment
//             of CensusVolArgs.seg rows.  It keeps the packed column sums of the strip's kCvTX + 2R window columns
//             in registers; per row step it adds the entering row's pixel costs (v_xor + v_bcnt, which
//             accumulates into the low half for free), subtracts the leaving row's, slides the
//             horizontal sum and stores one dword per lane (a full 256-B line per column).  A column
//             sum is at most 15 * 62 = 930 and a block cost at most 225 * 62 = 13,950, so the carry-free
//             packed add / subtract is exact.  The right codes of a row are staged in LDS in disparity
//             order (B[j] = T_R(cx(q0 + j))): lane l reads consecutive entries with aligned wide reads
//             and each entry serves two (column, disparity) terms; the left code of a column is a
//             broadcast LDS read.  The next step's codes are loaded from global memory into registers
//             before the current step's arithmetic, so their latency overlaps it.
// Algorithmic bytes per (pixel, d): 2 (the volume write); the codes are read 2R + 2 times per segment
// row from L2.
#include <type_traits>

#include "dsx_internal.h"

namespace dsx {

namespace {

constexpr int kCtTW = 64, kCtTH = 16;  // census_transform tile (256 threads, 4 rows per thread)
constexpr int kCvTX = 32;              // census_volume: columns per wave

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// OutT: uint64_t, or uint32_t (5x5 inside the handle)
template <int WX, int WY, class OutT>
__global__ __launch_bounds__(256) void census_transform(CensusArgs a) {
    constexpr int RX = WX / 2, RY = WY / 2;
    constexpr int TW = kCtTW + 2 * RX, TH = kCtTH + 2 * RY, TPW = TW / 4 + 1, TP = 4 * TPW;  // row pitch: dwords, bytes
    __shared__ uint32_t tile32[TH * TPW];
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile32);
    const int W = a.W, H = a.H, tid = threadIdx.x;
    const uint8_t *src = a.src[blockIdx.z];
    const int tx0 = blockIdx.x * kCtTW, ty0 = blockIdx.y * kCtTH;
    // stage: tile[ty][tx] = I(cx(tx0 - RX + tx), cy(ty0 - RY + ty)).  A wave owns every fourth tile
    // row, a lane the columns lane and lane + 64; all loads of a lane are issued before its first LDS
    // write so their latencies overlap
    {
        constexpr int kSR = (TH + 3) / 4, kSC = (TW + 63) / 64;
        uint8_t val[kSR][kSC];
#pragma unroll
        for (int i = 0; i < kSR; ++i) {
            const int ty = (tid >> 6) + 4 * i;
            const uint8_t *p = src + (int64_t)clampi(ty0 - RY + ty, 0, H - 1) * a.stride;
#pragma unroll
            for (int j = 0; j < kSC; ++j) {
                const int tx = (tid & 63) + 64 * j;
                val[i][j] = 0;
                if (ty < TH && tx < TW) val[i][j] = p[clampi(tx0 - RX + tx, 0, W - 1)];
            }
        }
#pragma unroll
        for (int i = 0; i < kSR; ++i) {
            const int ty = (tid >> 6) + 4 * i;
#pragma unroll
            for (int j = 0; j < kSC; ++j) {
                const int tx = (tid & 63) + 64 * j;
                if (ty < TH && tx < TW) tile[ty * TP + tx] = val[i][j];
            }
        }
    }
    __syncthreads();
    const int lx = tid & 63, x = tx0 + lx;
    if (x >= W) return;
    // A lane codes 4 consecutive rows of its column: their windows share 4 + WY - 1 tile rows.  Of each
    // row it reads the aligned dwords that hold its WX bytes (the 4 lanes of a dword group read the same
    // ones: a broadcast, no bank conflict; byte-addressed wide reads would be misaligned) and shifts
    // them into place with v_alignbyte_b32: win[row][n] = the window's bytes 4n .. 4n + 3
    constexpr int NR = 4 + WY - 1, ND = (WX + 6) / 4, NWD = (WX + 3) / 4;
    const int ly0 = (tid >> 6) * 4;
    const uint32_t sh = lx & 3;
    uint32_t win[NR][NWD];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const uint32_t *p = tile32 + (ly0 + r) * TPW + (lx >> 2);
        uint32_t d[ND + 1];
#pragma unroll
        for (int q = 0; q < ND; ++q) d[q] = p[q];
        d[ND] = 0;
#pragma unroll
        for (int n = 0; n < NWD; ++n) win[r][n] = __builtin_amdgcn_alignbyte(d[n + 1], d[n], sh);
    }
    OutT *dst = static_cast<OutT *>(a.dst[blockIdx.z]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = ty0 + ly0 + r;
        if (y >= H) break;
        const int c = (win[r + RY][RX / 4] >> (8 * (RX % 4))) & 0xFF;
        // the neighbours in reverse order, each shifted in from below: neighbour k ends at bit k
        uint32_t lo = 0, hi = 0;
        int k = WX * WY - 2;
#pragma unroll
        for (int j = WY - 1; j >= 0; --j) {
#pragma unroll
            for (int i = WX - 1; i >= 0; --i) {
                if (j == RY && i == RX) continue;
                const int nb = (win[r + j][i / 4] >> (8 * (i % 4))) & 0xFF;
                const uint32_t diff = (uint32_t)(nb - c);  // sign bit = neighbour < centre
                if (k >= 32) hi = __builtin_amdgcn_alignbit(hi, diff, 31);
                else lo = __builtin_amdgcn_alignbit(lo, diff, 31);
                --k;
            }
        }
        if constexpr (sizeof(OutT) == 8) dst[(int64_t)y * W + x] = (uint64_t)hi << 32 | lo;
        else dst[(int64_t)y * W + x] = lo;
    }
}

__device__ __forceinline__ uint32_t popc(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
__device__ __forceinline__ uint32_t popc(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }

template <class CT>
struct Pair {
    CT a, b;
};

// R: block radius; CT: code type (uint64_t 9x7, uint32_t 5x5); a.seg: rows per segment
template <int R, class CT>
__global__ __launch_bounds__(64) void census_volume(CensusVolArgs a) {
    constexpr int K = kCvTX + 2 * R;  // window columns of the strip (even)
    constexpr int NB = K + 128;       // staged right codes per row
    constexpr int NBL = (NB + 63) / 64;
    // [0]: the entering row, [1]: the leaving row
    __shared__ __attribute__((aligned(16))) CT sB[2][NB];
    __shared__ __attribute__((aligned(16))) CT sA[2][K];
    const int l = threadIdx.x;
    const int W = a.W, H = a.H, D = a.D, Dp = a.Dp;
    const int x0 = blockIdx.x * kCvTX, y0 = blockIdx.y * a.seg, dbase = blockIdx.z * 128;
    const int rows = min(a.seg, H - y0);
    const int d0 = dbase + 2 * l;
    const uint32_t pv = a.padv & 0xFFFFu;
    const uint32_t keep = (d0 < D ? 0xFFFFu : 0u) | (d0 + 1 < D ? 0xFFFF0000u : 0u);
    const uint32_t pad = (pv | pv << 16) & ~keep;
    const uint32_t lu = threadIdx.x;
    uint32_t *out = reinterpret_cast<uint32_t *>(a.vol) + (((int64_t)y0 * W + x0) * Dp + dbase) / 2;  // wave-uniform
    const int64_t ostep = Dp / 2;  // dwords per column
    const int ncols = min(kCvTX, W - x0);
    if (dbase >= D) {  // padding only: nothing to compute
        for (int y = 0; y < rows; ++y)
            for (int c = 0; c < ncols; ++c) (out + ((int64_t)y * W + c) * ostep)[lu] = pad;
        return;
    }
    const CT *TL = static_cast<const CT *>(a.codeL), *TR = static_cast<const CT *>(a.codeR);
    // B[j] = T_R(cx(q0 + j)): column k (position x0 - R + k) meets disparity d at j = k + 127 - (d - dbase)
    const int q0 = x0 - R - a.m - dbase - 127;
    int bx[NBL];
#pragma unroll
    for (int i = 0; i < NBL; ++i) bx[i] = clampi(q0 + l + 64 * i, 0, W - 1);
    const int ax = clampi(x0 - R + l, 0, W - 1);

    CT pb[2][NBL], pa[2];  // the next step's codes on their way from global memory
    const auto fetch = [&](int s) {
        // step s: row y0 - R + s enters, row y0 - R + s - (2R + 1) leaves (from step 2R + 1 on)
        const int64_t re = (int64_t)clampi(y0 - R + s, 0, H - 1) * W;
        const int64_t rl = (int64_t)clampi(y0 - 3 * R - 1 + s, 0, H - 1) * W;
#pragma unroll
        for (int i = 0; i < NBL; ++i) {
            pb[0][i] = TR[re + bx[i]];
            if (R > 0) pb[1][i] = TR[rl + bx[i]];
        }
        pa[0] = TL[re + ax];
        if (R > 0) pa[1] = TL[rl + ax];
    };
    const auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NBL; ++i) {
            if (l + 64 * i < NB) {
                sB[0][l + 64 * i] = pb[0][i];
                if (R > 0) sB[1][l + 64 * i] = pb[1][i];
            }
        }
        if (l < K) {
            sA[0][l] = pa[0];
            if (R > 0) sA[1][l] = pa[1];
        }
    };

    uint32_t cs[R > 0 ? K : 1];  // packed column sums (d0 low, d0 + 1 high)
    if (R > 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) cs[k] = 0;
    }
    const int nsteps = 2 * R + rows;
    fetch(0);
    for (int s = 0; s < nsteps; ++s) {
        __syncthreads();  // the previous step's reads are done
        stage();
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);
        const bool leave = R > 0 && s >= 2 * R + 1;
        const int j0 = 126 - 2 * l;  // column 0: d0 + 1 at j0, d0 at j0 + 1
        // the output row's first column: a wave-uniform pointer, the lane's dword added by the store
        uint32_t *orow = out + (int64_t)(s - 2 * R) * W * ostep;
        if constexpr (R == 0) {
            // full: all kCvTX columns lie inside the image (every strip but a ragged last one)
            const auto row = [&](auto full) {
                Pair<CT> e01 = *reinterpret_cast<const Pair<CT> *>(&sB[0][j0]);
#pragma unroll
                for (int k = 0; k < K; k += 2) {
                    const Pair<CT> e23 = *reinterpret_cast<const Pair<CT> *>(&sB[0][j0 + k + 2]);
                    const Pair<CT> al = *reinterpret_cast<const Pair<CT> *>(&sA[0][k]);
                    const uint32_t c0 = popc(al.a ^ e01.b) + (popc(al.a ^ e01.a) << 16);
                    const uint32_t c1 = popc(al.b ^ e23.a) + (popc(al.b ^ e01.b) << 16);
                    if (full.value || k < ncols) (orow + (int64_t)k * ostep)[lu] = (c0 & keep) | pad;
                    if (full.value || k + 1 < ncols) (orow + (int64_t)(k + 1) * ostep)[lu] = (c1 & keep) | pad;
                    e01 = e23;
                }
            };
            if (ncols == kCvTX) row(std::true_type{});
            else row(std::false_type{});
        } else {
            {
                Pair<CT> e01 = *reinterpret_cast<const Pair<CT> *>(&sB[0][j0]);
#pragma unroll
                for (int k = 0; k < K; k += 2) {
                    const Pair<CT> e23 = *reinterpret_cast<const Pair<CT> *>(&sB[0][j0 + k + 2]);
                    const Pair<CT> al = *reinterpret_cast<const Pair<CT> *>(&sA[0][k]);
                    cs[k] = (cs[k] + popc(al.a ^ e01.b)) + (popc(al.a ^ e01.a) << 16);
                    cs[k + 1] = (cs[k + 1] + popc(al.b ^ e23.a)) + (popc(al.b ^ e01.b) << 16);
                    e01 = e23;
                }
            }
            if (leave) {
                Pair<CT> e01 = *reinterpret_cast<const Pair<CT> *>(&sB[1][j0]);
#pragma unroll
                for (int k = 0; k < K; k += 2) {
                    const Pair<CT> e23 = *reinterpret_cast<const Pair<CT> *>(&sB[1][j0 + k + 2]);
                    const Pair<CT> al = *reinterpret_cast<const Pair<CT> *>(&sA[1][k]);
                    cs[k] -= popc(al.a ^ e01.b) | (popc(al.a ^ e01.a) << 16);
                    cs[k + 1] -= popc(al.b ^ e23.a) | (popc(al.b ^ e01.b) << 16);
                    e01 = e23;
                }
            }
            if (s >= 2 * R) {
                const auto row = [&](auto full) {
                    uint32_t h = 0;
#pragma unroll
                    for (int k = 0; k < 2 * R; ++k) h += cs[k];
#pragma unroll
                    for (int c = 0; c < kCvTX; ++c) {
                        h += cs[c + 2 * R];
                        if (full.value || c < ncols) (orow + (int64_t)c * ostep)[lu] = (h & keep) | pad;
                        h -= cs[c];
                    }
                };
                if (ncols == kCvTX) row(std::true_type{});
                else row(std::false_type{});
            }
        }
    }
}

template <int R, class CT>
hipError_t launch_cv_r(const CensusVolArgs &a, hipStream_t st) {
    const dim3 grid((a.W + kCvTX - 1) / kCvTX, (a.H + a.seg - 1) / a.seg, a.Dp / 128);
    hipLaunchKernelGGL((census_volume<R, CT>), grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

template <class CT>
hipError_t launch_cv(const CensusVolArgs &a, hipStream_t st) {
    switch (a.R) {
        case 0: return launch_cv_r<0, CT>(a, st);
        case 1: return launch_cv_r<1, CT>(a, st);
        case 2: return launch_cv_r<2, CT>(a, st);
        case 3: return launch_cv_r<3, CT>(a, st);
        case 4: return launch_cv_r<4, CT>(a, st);
        case 5: return launch_cv_r<5, CT>(a, st);
        case 6: return launch_cv_r<6, CT>(a, st);
        case 7: return launch_cv_r<7, CT>(a, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

size_t census_code_bytes(int window) { return window == kCensus9x7 ? 8 : 4; }

hipError_t launch_census_transform(const CensusArgs &a, hipStream_t st) {
    if (a.nviews < 1 || a.nviews > 2 || a.H < 1 || a.W < 1 || (a.H + kCtTH - 1) / kCtTH > 65535)
        return hipErrorInvalidValue;
    const dim3 grid((a.W + kCtTW - 1) / kCtTW, (a.H + kCtTH - 1) / kCtTH, a.nviews);
    if (a.window == kCensus9x7) {
        if (!a.out64) return hipErrorInvalidValue;
        hipLaunchKernelGGL((census_transform<9, 7, uint64_t>), grid, dim3(256), 0, st, a);
    } else if (a.window == kCensus5x5) {
        if (a.out64) hipLaunchKernelGGL((census_transform<5, 5, uint64_t>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((census_transform<5, 5, uint32_t>), grid, dim3(256), 0, st, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_census_volume(const CensusVolArgs &a, hipStream_t st) {
    if (a.Dp % 128 != 0 || a.H < 1 || a.W < 1 || a.D < 1 || a.D > a.Dp)
        return hipErrorInvalidValue;
    CensusVolArgs k = a;
    if (k.seg <= 0) k.seg = kCensusSeg;
    if ((a.H + k.seg - 1) / k.seg > 65535) return hipErrorInvalidValue;
    if (a.window == kCensus9x7) return launch_cv<uint64_t>(k, st);
    if (a.window == kCensus5x5) return launch_cv<uint32_t>(k, st);
    return hipErrorInvalidValue;
}

}  // namespace dsx
