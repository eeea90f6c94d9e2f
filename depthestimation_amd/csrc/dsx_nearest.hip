// Hole filling by iterated dilation: fill_holes(method='nearest') (depthlib/postprocess.py:106-116;
// host restatement depthestimation_amd/postprocess.py fill_holes / nearest_footprint):
//
//   mask = d <= 0 (from the INPUT, fixed);  r = k / 2;  E = the ellipse footprint of radius r
//   f_0 = d;  k times:  f_{t+1}(p) = mask(p) ? max over q in p + E of f_t(q) : f_t(p)
//
// The host's replicated border equals skipping the taps outside the image for these footprints
// (clamping a disc offset towards the centre stays inside the disc), so out-of-image cells are
// -inf here and never holes.  The only arithmetic is a float max: no rounding, bit-exact with the
// host.  The kernels see the footprint as per-row half-widths (hw[dy + r], -1 = empty row) written
// by nearest_footprint below, the one C home of the ellipse rule.
//
// Two paths, block barriers only (no grid barrier, no atomics, no host readback, no state):
//
//   nearest_fused  all k iterations of one output tile in LDS.  The block loads the tile plus a
//     halo of h = k r into two float tiles A and B (the same values: only holes are ever rewritten,
//     so a non-hole cell is already right in both), iterates A -> B -> A ..., then writes the tile.
//     Iteration t (0-based) only has to be right on the tile grown by (k - 1 - t) r, and reads the
//     tile grown by (k - t) r, which iteration t - 1 left right; its last reads touch row / column 0
//     and kPW - 1 / PH - 1 of the padded tile, never beyond.  The thread -> cell map is the same in
//     every iteration (wave w owns rows w, w + 8, ...; lane l owns columns l and l + 64), so each
//     thread keeps the hole mask of its <= 14 cells as bits of one register, and a wave whose cells
//     hold no hole issues no LDS read.  A block whose padded tile holds no hole (__syncthreads_or)
//     copies through without iterating.  Latency is what this kernel pays, so each phase issues all
//     of its reads before it uses the first: the 14 global loads of a thread (addresses clamped into
//     the image, out-of-image values dropped afterwards), a hole's (2 r + 1)^2 window (the kernel is
//     built per radius 0, 1, 2; the half-widths stay run-time values that mask the window), and the
//     LDS reads of the write-out.
//
//     LDS arithmetic.  Padded tile kPW x PH floats, kPW = 128 fixed, PH = kTY + 2 h, kTY = 32:
//     the output tile is (128 - 2 h) x 32.  A row read is 64 lanes at consecutive dwords (and the
//     taps are the same run shifted by dx), so every ds_read_b32 / ds_write_b32 32-lane group covers 32
//     distinct banks whatever the row stride: 128 needs no padding.  Two tiles = 1024 PH bytes:
//       k <= 1 : h = 0,  PH = 32, 32 KiB, tile 128 x 32   (no iteration: a copy)
//       k 2, 3 : h = 2/3, PH = 36/38, 36/38 KiB, 4 blocks per CU (160 KiB), 32 waves
//       k 4, 5 : h = 8/10, PH = 48/52, 48/52 KiB, 3 blocks per CU, 24 waves; loads 1.9x the tile
//       k 6, 7 : h = 18/21, PH = 68/74, 68/74 KiB: past the 64 KiB of a plain dynamic-LDS launch,
//                2 blocks per CU and 2.8x / 3.4x the tile loaded - not worth it.
//     So kNearestFusedMaxK = 5 (the reference's fill_kernel 3 and fill_holes' default 5), 512
//     threads: 8 waves x 7 rows cover PH <= 56.
//
//   nearest_step  one iteration per launch, global -> global, any k <= 31: the mask comes from the
//     original input, the source alternates between the workspace and the output so that the last
//     iteration lands in the output.  k <= 1 runs one identity step (the copy).
#include "dsx_internal.h"

namespace dsx {

#pragma clang fp contract(off)

// Half-widths of the footprint rows, hw[dy + r] for dy in [-r, r] (-1: empty row).  The rule is
// numpy's: (dy / r)^2 + (dx / r)^2 <= 1.0 in float64, each quotient rounded, squared, the squares
// added - no contraction, no integer shortcut (at r = 13 the two differ in 8 cells).
int nearest_footprint(int k, int32_t *hw, int cap) {
    if (k < 0 || k > kNearestMaxK || !hw) return -1;
    const int r = k / 2, n = 2 * r + 1;
    if (cap < n) return -1;
    if (r == 0) {
        hw[0] = 0;
        return 1;
    }
    for (int dy = -r; dy <= r; ++dy) {
        int w = -1;
        const volatile double a = (double)dy / (double)r;
        const volatile double a2 = a * a;
        for (int dx = 0; dx <= r; ++dx) {
            const volatile double b = (double)dx / (double)r;
            const volatile double b2 = b * b;
            const volatile double s = a2 + b2;
            if (s <= 1.0) w = dx;
        }
        hw[dy + r] = w;
    }
    return n;
}

size_t nearest_workspace(int H, int W) {
    return (((size_t)H * (size_t)W * 4) + 255) & ~(size_t)255;
}

namespace {

constexpr int kPW = 128;      // padded tile width (two 64-lane row segments)
constexpr int kTY = 32;       // output tile height
constexpr int kFThreads = 512;
constexpr int kFWaves = kFThreads / 64;
constexpr int kFRows = 7;     // rows per wave: 8 * 7 = 56 >= kTY + 2 * 10
static_assert(kFWaves * kFRows >= kTY + 2 * kNearestFusedMaxK * (kNearestFusedMaxK / 2), "padded rows");

struct Footprint {
    int r;
    int hw[kNearestMaxK];  // r <= 15: 31 rows
};

// R: the footprint radius (rows 2 R + 1), the one thing fixed at compile time: a hole's (2 R + 1)^2
// window reads are issued together and the cells beyond a row's half-width drop out of the max, so
// the LDS latency is paid once per hole and iteration, not once per tap.
template <int R>
__global__ __launch_bounds__(kFThreads) void nearest_fused(const float *__restrict__ in, int64_t pitch, int H, int W,
                                                            int iters, Footprint fp, float *__restrict__ out) {
    extern __shared__ float tile[];
    constexpr int r = R;
    int hw[2 * R + 1];
#pragma unroll
    for (int i = 0; i < 2 * R + 1; ++i) hw[i] = fp.hw[i];
    const int h = iters * r;
    const int TX = kPW - 2 * h, PH = kTY + 2 * h;
    float *A = tile, *B = tile + kPW * PH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * TX - h, y0 = blockIdx.y * kTY - h;
    const float ninf = -__builtin_inff();

    // every cell's load goes out before the first one is used: the address is clamped into the image
    // (always readable), and a cell outside it, or below the padded tile, drops the value afterwards
    float v[kFRows][2];
#pragma unroll
    for (int j = 0; j < kFRows; ++j) {
        const int gy = y0 + wave + kFWaves * j;
        const int cy = gy < 0 ? 0 : gy >= H ? H - 1 : gy;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int gx = x0 + lane + 64 * c;
            const int cx = gx < 0 ? 0 : gx >= W ? W - 1 : gx;
            v[j][c] = in[(int64_t)cy * pitch + cx];
        }
    }
    unsigned bits = 0;  // bit j * 2 + c: the cell (wave + 8 j, lane + 64 c) is a hole
#pragma unroll
    for (int j = 0; j < kFRows; ++j) {
        const int row = wave + kFWaves * j;
        const int gy = y0 + row;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int col = lane + 64 * c;
            const int gx = x0 + col;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W && row < PH;
            const float val = inside ? v[j][c] : ninf;
            if (inside && val <= 0.0f) bits |= 1u << (j * 2 + c);
            if (row < PH) {
                A[row * kPW + col] = val;
                B[row * kPW + col] = val;
            }
        }
    }
    const int any = __syncthreads_or(bits != 0);  // also orders the loads before the first reads

    const float *fin = A;
    if (any) {
        float *src = A, *dst = B;
        for (int t = 0; t < iters; ++t) {
            const int g = (iters - 1 - t) * r;  // this iteration is needed on the tile grown by g
            if (bits) {
#pragma unroll
                for (int j = 0; j < kFRows; ++j) {
                    const int row = wave + kFWaves * j;
                    if (row < h - g || row >= h + kTY + g) continue;
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int col = lane + 64 * c;
                        if (!((bits >> (j * 2 + c)) & 1u) || col < h - g || col >= h + TX + g) continue;
                        const float *p = src + row * kPW + col;
                        float m = ninf;
#pragma unroll
                        for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                            for (int dx = -R; dx <= R; ++dx) {
                                const float tap = p[dy * kPW + dx];  // inside the padded tile for every |dx| <= R
                                m = fmaxf(m, (dx < 0 ? -dx : dx) <= hw[dy + R] ? tap : ninf);
                            }
                        }
                        dst[row * kPW + col] = m;
                    }
                }
            }
            __syncthreads();
            float *s = src;
            src = dst;
            dst = s;
        }
        fin = src;
    }

    // the same for the way out: the LDS reads first (row clamped into the padded tile), then the stores
#pragma unroll
    for (int j = 0; j < kFRows; ++j) {
        const int row = wave + kFWaves * j;
#pragma unroll
        for (int c = 0; c < 2; ++c) v[j][c] = fin[(row < PH ? row : PH - 1) * kPW + lane + 64 * c];
    }
#pragma unroll
    for (int j = 0; j < kFRows; ++j) {
        const int row = wave + kFWaves * j;
        const int gy = y0 + row;
        if (row < h || row >= h + kTY || gy >= H) continue;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int col = lane + 64 * c;
            const int gx = x0 + col;
            if (col < h || col >= h + TX || gx >= W) continue;
            out[(int64_t)gy * W + gx] = v[j][c];
        }
    }
}

constexpr int kSX = 64, kSY = 4;  // nearest_step block: 64 x 4 pixels, one per thread

__global__ __launch_bounds__(kSX * kSY) void nearest_step(const float *__restrict__ in, int64_t in_pitch,
                                                           const float *__restrict__ src, int64_t src_pitch, int H,
                                                           int W, Footprint fp, float *__restrict__ dst) {
    const int x = blockIdx.x * kSX + (threadIdx.x & (kSX - 1));
    const int y = blockIdx.y * kSY + (threadIdx.x / kSX);
    if (x >= W || y >= H) return;
    float v = src[(int64_t)y * src_pitch + x];
    if (in[(int64_t)y * in_pitch + x] <= 0.0f) {
        const int r = fp.r;
        for (int dy = -r; dy <= r; ++dy) {
            const int w = fp.hw[dy + r];
            const int yy = y + dy;
            if (w < 0 || yy < 0 || yy >= H) continue;
            const int xa = x - w < 0 ? 0 : x - w, xb = x + w >= W ? W - 1 : x + w;
            const float *p = src + (int64_t)yy * src_pitch;
            for (int xx = xa; xx <= xb; ++xx) v = fmaxf(v, p[xx]);
        }
    }
    dst[(int64_t)y * W + x] = v;
}

}  // namespace

hipError_t launch_nearest(const float *in, int64_t pitch, int H, int W, int k, float *out, float *ws, int path,
                          hipStream_t st) {
    int32_t hw[kNearestMaxK];
    const int rows = nearest_footprint(k, hw, kNearestMaxK);
    if (rows < 0) return hipErrorInvalidValue;
    Footprint fp{};
    fp.r = rows / 2;
    for (int i = 0; i < rows; ++i) fp.hw[i] = hw[i];
    const int iters = fp.r == 0 ? 0 : k;  // a one-pixel footprint changes nothing
    if (path == kNearestFused) {
        if (k > kNearestFusedMaxK) return hipErrorInvalidValue;
        const int h = iters * fp.r;
        const int TX = kPW - 2 * h, PH = kTY + 2 * h;
        const dim3 grid((W + TX - 1) / TX, (H + kTY - 1) / kTY);
        if (grid.y > 65535u) return hipErrorInvalidValue;
        static_assert(kNearestFusedMaxK / 2 == 2, "nearest_fused is built for radius 0, 1 and 2");
        auto kern = fp.r == 0 ? nearest_fused<0> : fp.r == 1 ? nearest_fused<1> : nearest_fused<2>;
        hipLaunchKernelGGL(kern, grid, dim3(kFThreads), (size_t)2 * kPW * PH * sizeof(float), st, in, pitch, H, W, iters,
                           fp, out);
        return hipGetLastError();
    }
    const int steps = iters > 0 ? iters : 1;
    if (steps > 1 && !ws) return hipErrorInvalidValue;
    const dim3 grid((W + kSX - 1) / kSX, (H + kSY - 1) / kSY);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    const float *src = in;
    int64_t sp = pitch;
    for (int i = 0; i < steps; ++i) {
        float *dst = ((steps - 1 - i) & 1) ? ws : out;  // the last step writes the output
        hipLaunchKernelGGL(nearest_step, grid, dim3(kSX * kSY), 0, st, in, pitch, src, sp, H, W, fp, dst);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        src = dst;
        sp = W;
    }
    return hipSuccess;
}

}  // namespace dsx
