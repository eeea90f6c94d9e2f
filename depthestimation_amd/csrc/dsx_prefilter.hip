// Matcher prefilter and texture threshold (include/dsx.h dsx_prefilter): streaming uint8 stencils in
// front of and behind the block-matching passes.  DESIGN.md section 4.3d has the contract and the times.
//
//   xsobel       : P = clip(Sx, -c, c) + c, Sx the 3x3 x-Sobel with rows clamped; columns 0 and W-1
//                  hold c (channel 0 of oracle/bt_cost.py with ftzero = c).
//   mean         : P = clip(I - mu, -c, c) + c, mu = (S + n*n/2) / (n*n), S the n x n box sum with
//                  clamped coordinates.
//   texture sum  : T = block x block box sum of |P - c| with clamped coordinates; the mask form writes
//                  the matcher's invalid value where T < t.
//
// xsobel: a lane owns 16 columns of kXsRows consecutive rows, keeps the horizontal differences of three
// rows in registers and writes 16 bytes per row with one store.  mean / texture: one block stages a
// (32 + n - 1) x (128 + n - 1) tile in LDS (clamped byte loads, all independent), runs the column sums
// down the tile (one lane per column, running add / subtract), then slides the row sums over 16
// outputs per lane.
#include <hip/hip_runtime.h>

#include "dsx_internal.h"

namespace dsx {
namespace {

constexpr int kXsRows = 2;     // rows per xsobel lane: 4 row loads per 2 output rows, two waves per SIMD at 1080p
constexpr int kTH = 32;        // box tile: output rows
constexpr int kTW = 128;       // box tile: output columns (8 lanes x 16)
constexpr int kMaxN = 21;      // largest window (prefilter_size; block_size <= 15)
constexpr int kTP = 156;       // tile pitch in bytes: >= kTW + kMaxN - 1, an odd number of dwords
constexpr int kVP = 154;       // column-sum pitch in u16: >= kTW + kMaxN - 1, an odd number of dwords

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void store16(uint8_t *p, const int (&o)[16], bool wide, int nvalid) {
    if (wide) {
        uint4 q;
        q.x = (uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16 | (uint32_t)o[3] << 24;
        q.y = (uint32_t)o[4] | (uint32_t)o[5] << 8 | (uint32_t)o[6] << 16 | (uint32_t)o[7] << 24;
        q.z = (uint32_t)o[8] | (uint32_t)o[9] << 8 | (uint32_t)o[10] << 16 | (uint32_t)o[11] << 24;
        q.w = (uint32_t)o[12] | (uint32_t)o[13] << 8 | (uint32_t)o[14] << 16 | (uint32_t)o[15] << 24;
        *reinterpret_cast<uint4 *>(p) = q;
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < nvalid) p[i] = (uint8_t)o[i];
    }
}

// SAL: every source row starts 16-B aligned (base and stride), so a lane's 16 source bytes are one
// aligned load; otherwise the same 16 bytes come from a byte-addressed copy.  The last lane of a row
// (fewer than 16 columns left) reads its bytes one by one, clamped into the row.
template <bool SAL>
__global__ __launch_bounds__(256) void xsobel_kernel(PrefilterArgs a) {
    const int W = a.W, H = a.H;
    const int nx = (W + 15) >> 4, ny = (H + kXsRows - 1) / kXsRows;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= nx * ny) return;
    const int gy = u / nx, lx = u - gy * nx;
    const int v = blockIdx.y % a.nviews, f = blockIdx.y / a.nviews;
    const uint8_t *src = a.src[v] + (int64_t)f * a.frame_stride;
    uint8_t *dst = a.dst[v] + (int64_t)f * a.dframe;
    const int x0 = lx * 16, y0 = gy * kXsRows;
    const bool full = x0 + 16 <= W;                            // 16 source bytes inside the row
    const bool wide = a.dal && x0 + 16 <= a.dwidth;            // 16 writable, aligned output bytes
    const int nvalid = W - x0 < 16 ? W - x0 : 16;
    const int c = a.cap;

    // d[i] = I(x0 + i + 1, y) - I(x0 + i - 1, y); the neighbours of columns 0 and W-1 are clamped
    // (those two outputs are replaced by c below)
    auto diffs = [&](int y, int (&d)[16]) {
        const uint8_t *p = src + (int64_t)y * a.stride;
        int b[18];
        if (full) {
            uint4 q;
            if (SAL) q = *reinterpret_cast<const uint4 *>(p + x0);
            else __builtin_memcpy(&q, p + x0, 16);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) b[i + 1] = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu);
            b[0] = p[x0 > 0 ? x0 - 1 : 0];
            b[17] = p[x0 + 16 < W ? x0 + 16 : W - 1];
        } else {
#pragma unroll
            for (int i = 0; i < 18; ++i) b[i] = p[clampi(x0 - 1 + i, 0, W - 1)];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = b[i + 2] - b[i];
    };

    int up[16], mid[16], dn[16];
    diffs(y0 > 0 ? y0 - 1 : 0, up);
    diffs(y0, mid);
#pragma unroll
    for (int r = 0; r < kXsRows; ++r) {
        const int y = y0 + r;
        if (y >= H) break;
        diffs(y + 1 < H ? y + 1 : H - 1, dn);
        int o[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int x = x0 + i;
            const int s = clampi(2 * mid[i] + up[i] + dn[i], -c, c) + c;
            o[i] = (x == 0 || x >= W - 1) ? c : s;
        }
        store16(dst + (int64_t)y * a.dpitch + x0, o, wide, nvalid);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            up[i] = mid[i];
            mid[i] = dn[i];
        }
    }
}

enum { BOX_MEAN = 0, BOX_TSUM = 1, BOX_TMASK = 2 };

struct BoxArgs {
    const uint8_t *src[2];  // per view; frame f at + f * frame_stride
    int64_t stride, frame_stride;
    int nviews, H, W;
    int n;                  // window (odd, <= kMaxN)
    int cap;
    uint32_t magic;         // BOX_MEAN: floor(2^32 / n^2) + 1, so umulhi(s, magic) = s / n^2 for s < 2^17
    // BOX_MEAN output
    uint8_t *dst[2];
    int64_t dpitch, dframe;
    int dwidth, dal;
    // BOX_TSUM / BOX_TMASK outputs: contiguous H x W per frame
    uint16_t *out_sum;
    int16_t *out_fixed;
    float *out_float;
    int thr, inv16;
    float invf;
};

template <int MODE>
__global__ __launch_bounds__(256) void box_kernel(BoxArgs a) {
    __shared__ uint8_t tile[(kTH + kMaxN - 1) * kTP];
    __shared__ uint16_t vs[kTH * kVP];
    const int W = a.W, H = a.H, n = a.n, hr = n >> 1, c = a.cap;
    const int tid = threadIdx.x;
    const int v = blockIdx.z % a.nviews, f = blockIdx.z / a.nviews;
    const uint8_t *src = a.src[v] + (int64_t)f * a.frame_stride;
    const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
    const int tw = kTW + n - 1, th = kTH + n - 1;

    // stage: tile[ty][tx] = g(I(cx(tx0 - hr + tx), cy(ty0 - hr + ty))), g = identity or |. - c|.  A wave
    // owns every fourth tile row, a lane the columns lane, lane + 64, lane + 128; all loads of a lane
    // are issued before the first LDS write (fixed trip counts, predicated) so their latencies overlap
    {
        constexpr int kSR = (kTH + kMaxN - 1 + 3) / 4, kSC = (kTW + kMaxN - 1 + 63) / 64;
        uint8_t val[kSR][kSC];
#pragma unroll
        for (int i = 0; i < kSR; ++i) {
            const int ty = (tid >> 6) + 4 * i;
            const uint8_t *p = src + (int64_t)clampi(ty0 - hr + ty, 0, H - 1) * a.stride;
#pragma unroll
            for (int j = 0; j < kSC; ++j) {
                const int tx = (tid & 63) + 64 * j;
                val[i][j] = 0;
                if (ty < th && tx < tw) val[i][j] = p[clampi(tx0 - hr + tx, 0, W - 1)];
            }
        }
#pragma unroll
        for (int i = 0; i < kSR; ++i) {
            const int ty = (tid >> 6) + 4 * i;
#pragma unroll
            for (int j = 0; j < kSC; ++j) {
                const int tx = (tid & 63) + 64 * j;
                int v8 = val[i][j];
                if (MODE != BOX_MEAN) v8 = v8 > c ? v8 - c : c - v8;
                if (ty < th && tx < tw) tile[ty * kTP + tx] = (uint8_t)v8;
            }
        }
    }
    __syncthreads();
    // column sums: lane tx walks down its column (n rows enter, then one in / one out per row); the
    // row loop is unrolled so the reads of several rows are in flight together
    if (tid < tw) {
        int s = 0;
        for (int j = 0; j < n; ++j) s += tile[j * kTP + tid];
        vs[tid] = (uint16_t)s;
        const uint8_t *in = tile + (n - 1) * kTP + tid, *out = tile + tid;
#pragma unroll 8
        for (int r = 1; r < kTH; ++r) {
            s += (int)in[r * kTP] - (int)out[(r - 1) * kTP];
            vs[r * kVP + tid] = (uint16_t)s;
        }
    }
    __syncthreads();
    // row sums: lane (r, seg) slides the window over 16 outputs
    const int r = tid & 31, seg = tid >> 5;
    const int y = ty0 + r, x0 = tx0 + seg * 16;
    if (y >= H || x0 >= W) return;
    const uint16_t *vr = vs + r * kVP + seg * 16;
    int s = 0;
    for (int k = 0; k < n; ++k) s += vr[k];
    int o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        o[i] = s;
        if (i < 15) s += (int)vr[i + n] - (int)vr[i];
    }
    const int nvalid = W - x0 < 16 ? W - x0 : 16;
    const int64_t fo = (int64_t)f * H * W + (int64_t)y * W + x0;
    if (MODE == BOX_MEAN) {
        const uint8_t *ctr = tile + (r + hr) * kTP + seg * 16 + hr;
        const uint32_t half = (uint32_t)(n * n) >> 1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int mu = (int)__umulhi((uint32_t)o[i] + half, a.magic);
            o[i] = clampi((int)ctr[i] - mu, -c, c) + c;
        }
        uint8_t *dst = a.dst[v] + (int64_t)f * a.dframe + (int64_t)y * a.dpitch + x0;
        store16(dst, o, a.dal && x0 + 16 <= a.dwidth, nvalid);
    } else if (MODE == BOX_TSUM) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < nvalid) a.out_sum[fo + i] = (uint16_t)o[i];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < nvalid && o[i] < a.thr) {
                if (a.out_fixed) a.out_fixed[fo + i] = (int16_t)a.inv16;
                if (a.out_float) a.out_float[fo + i] = a.invf;
            }
        }
    }
}

bool aligned16(const void *p, int64_t pitch) { return ((uintptr_t)p & 15) == 0 && (pitch & 15) == 0; }

}  // namespace

hipError_t launch_prefilter(const PrefilterArgs &a, hipStream_t st) {
    PrefilterArgs k = a;
    bool dal = true, sal = (a.frame_stride & 15) == 0;
    for (int v = 0; v < a.nviews; ++v) {
        dal = dal && aligned16(a.dst[v], a.dpitch);
        sal = sal && aligned16(a.src[v], a.stride);
    }
    k.dal = dal && (a.dframe & 15) == 0;
    const int nz = a.nviews * a.nframes;
    if (nz < 1 || nz > 65535) return hipErrorInvalidValue;
    if (a.type == kPrefXsobel) {
        const int64_t units = (int64_t)((a.W + 15) >> 4) * ((a.H + kXsRows - 1) / kXsRows);
        const dim3 grid((unsigned)((units + 255) / 256), (unsigned)nz);
        if (sal) hipLaunchKernelGGL(xsobel_kernel<true>, grid, dim3(256), 0, st, k);
        else hipLaunchKernelGGL(xsobel_kernel<false>, grid, dim3(256), 0, st, k);
        return hipGetLastError();
    }
    if (a.n < 1 || a.n > kMaxN || (a.n & 1) == 0 || (a.H + kTH - 1) / kTH > 65535) return hipErrorInvalidValue;
    BoxArgs b{};
    for (int v = 0; v < a.nviews; ++v) {
        b.src[v] = a.src[v];
        b.dst[v] = a.dst[v];
    }
    b.stride = a.stride;
    b.frame_stride = a.frame_stride;
    b.nviews = a.nviews;
    b.H = a.H;
    b.W = a.W;
    b.n = a.n;
    b.cap = a.cap;
    b.magic = (uint32_t)((1ull << 32) / (uint64_t)(a.n * a.n)) + 1u;
    b.dpitch = a.dpitch;
    b.dframe = a.dframe;
    b.dwidth = a.dwidth;
    b.dal = k.dal;
    const dim3 grid((unsigned)((a.W + kTW - 1) / kTW), (unsigned)((a.H + kTH - 1) / kTH), (unsigned)nz);
    hipLaunchKernelGGL(box_kernel<BOX_MEAN>, grid, dim3(256), 0, st, b);
    return hipGetLastError();
}

hipError_t launch_texture(const TextureArgs &a, hipStream_t st) {
    if (a.block < 1 || a.block > 15 || (a.block & 1) == 0 || a.nframes < 1 || a.nframes > 65535 ||
        (a.H + kTH - 1) / kTH > 65535)
        return hipErrorInvalidValue;
    BoxArgs b{};
    b.src[0] = a.pref;
    b.stride = a.stride;
    b.frame_stride = a.frame_stride;
    b.nviews = 1;
    b.H = a.H;
    b.W = a.W;
    b.n = a.block;
    b.cap = a.cap;
    b.out_sum = a.out_sum;
    b.out_fixed = a.out_fixed;
    b.out_float = a.out_float;
    b.thr = a.thr;
    b.inv16 = a.inv16;
    b.invf = a.invf;
    const dim3 grid((unsigned)((a.W + kTW - 1) / kTW), (unsigned)((a.H + kTH - 1) / kTH), (unsigned)a.nframes);
    if (a.out_sum) hipLaunchKernelGGL(box_kernel<BOX_TSUM>, grid, dim3(256), 0, st, b);
    else hipLaunchKernelGGL(box_kernel<BOX_TMASK>, grid, dim3(256), 0, st, b);
    return hipGetLastError();
}

}  // namespace dsx
