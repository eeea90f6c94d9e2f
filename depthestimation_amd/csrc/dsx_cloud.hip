// Point-cloud output (dsx_cloud of dsx.h; host restatement depthestimation_amd/pointcloud.py): a finished
// float32 disparity map d (H x W, column 0 = image column x0) to metric XYZ.  Per pixel, all in float32,
// every operation correctly rounded and uncontracted:
//
//   adj = d + doffs;  Z = fB / adj;  valid = adj > eps && 0 < Z < inf && (!has_max || Z <= max_depth)
//   s = Z / f;  X = ((float)(x + x0) - cx) * s;  Y = ((float)y - cy) * s
//
// cloud_reproject writes the organized H x W x 3 map (NaN at invalid pixels), 256 pixels per block, its 768
// floats staged in LDS so that consecutive lanes store consecutive dwords.
//
// The compact cloud - the valid points in row-major pixel order, equal to the host's xyz[mask] - takes three
// launches and no block ever waits on another (no atomics, no look-back, no grid barrier):
//   cloud_count    a block owns a tile of kCT consecutive pixels; round r of 8 gives thread t pixel
//                  tile * kCT + r * 256 + t (a wave reads 256 consecutive bytes); ballot + popcount per
//                  wave and round, the 4 wave totals meet in LDS; one int per tile into the workspace
//   cloud_scan     one 1024-thread block turns the tile counts into exclusive offsets in place (chunks of
//                  1024 tiles with a running carry) and writes the total N to the caller's count word
//   cloud_scatter  recomputes the tile: the rank of a valid pixel is the sum of the (round, wave) counts
//                  before its own - 32 counts in LDS, every thread sums them - plus mbcnt of its wave's
//                  ballot below its lane.  The tile's output is the contiguous range [off, off + n) of the
//                  point list: 3 n floats, 3 n bytes, n ints.  Every lane stores its own point there (three
//                  dwords 12 bytes apart, three bytes, one int): the valid lanes of a wave fill one run of
//                  addresses between them.  DSX_CLOUD_STAGED builds the other form, which stages the tile's
//                  output in LDS by rank (39 KB) and stores it as consecutive dwords from consecutive lanes
//                  (the bytes as the aligned dwords of their global range, head and tail bytes singly); it
//                  measured 4-11 % slower.
// A point of rank >= cap is not written; the count stays the true N.
#include "dsx_internal.h"

#include <cmath>
#include <string>

#include "../../include/dsx.h"

#ifndef DSX_CLOUD_STAGED  // 1: LDS-staged stores instead of the lane-per-point ones (measured: DESIGN 4.4)
#define DSX_CLOUD_STAGED 0
#endif

namespace dsx {
int set_error(int code, const std::string &msg);  // dsx_api.hip: the message behind dsx_last_error
}

namespace {

constexpr int kCT = DSX_CLOUD_TILE, kCThreads = 256, kCWaves = kCThreads / 64;
constexpr int kCRounds = kCT / kCThreads;
constexpr int kScanThreads = 1024, kScanWaves = kScanThreads / 64;
static_assert(kCT % kCThreads == 0 && kCThreads % 64 == 0, "a tile is whole rounds of whole waves");

struct CloudArgs {
    const float *disp;
    int64_t pitch;       // elements
    uint32_t W, npix;    // H * W <= 2^31 - 1
    float fB, f, cx, cy, doffs, eps, max_depth;
    int has_max, x0;
};

#pragma clang fp contract(off)

// Z and its validity; NaN fails every comparison
__device__ __forceinline__ bool cloud_z(const CloudArgs &a, float d, float &Z) {
    const float adj = d + a.doffs;
    Z = __fdiv_rn(a.fB, adj);
    return adj > a.eps && Z > 0.0f && Z < __builtin_inff() && (!a.has_max || Z <= a.max_depth);
}

__device__ __forceinline__ void cloud_xy(const CloudArgs &a, uint32_t x, uint32_t y, float Z, float &X, float &Y) {
    const float s = __fdiv_rn(Z, a.f);
    X = ((float)(int)(x + (uint32_t)a.x0) - a.cx) * s;
    Y = ((float)(int)y - a.cy) * s;
}

#pragma clang fp contract(on)

// pixel p of the row-major H x W map: its value, honouring the pitch (p < npix)
__device__ __forceinline__ float cloud_load(const CloudArgs &a, uint32_t p, uint32_t &x, uint32_t &y) {
    y = p / a.W;
    x = p - y * a.W;
    return a.disp[(int64_t)y * a.pitch + x];
}

__global__ __launch_bounds__(kCThreads) void cloud_reproject(CloudArgs a, float *__restrict__ xyz) {
    __shared__ float sp[3 * kCThreads];
    const int tid = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)kCThreads, p = base + tid;
    const float nan = __uint_as_float(0x7FC00000u);
    float X = nan, Y = nan, Z = nan;
    if (p < a.npix) {
        uint32_t x, y;
        float z;
        if (cloud_z(a, cloud_load(a, p, x, y), z)) {
            Z = z;
            cloud_xy(a, x, y, z, X, Y);
        }
    }
    sp[3 * tid] = X;
    sp[3 * tid + 1] = Y;
    sp[3 * tid + 2] = Z;
    __syncthreads();
    const uint32_t n = min((uint32_t)kCThreads, a.npix - base) * 3u;
    float *out = xyz + 3 * (int64_t)base;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t i = k * kCThreads + tid;
        if (i < n) out[i] = sp[i];
    }
}

__global__ __launch_bounds__(kCThreads) void cloud_count(CloudArgs a, int *__restrict__ tiles) {
    __shared__ int wc[kCWaves];
    const int tid = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)kCT;
    int n = 0;
#pragma unroll
    for (int r = 0; r < kCRounds; ++r) {
        const uint32_t p = base + r * kCThreads + tid;
        bool v = false;
        if (p < a.npix) {
            uint32_t x, y;
            float z;
            // the count needs no coordinates: a contiguous map is read without the division
            v = cloud_z(a, a.pitch == (int64_t)a.W ? a.disp[p] : cloud_load(a, p, x, y), z);
        }
        n += __popcll(__ballot(v));
    }
    if ((tid & 63) == 0) wc[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kCWaves; ++w) s += wc[w];
        tiles[blockIdx.x] = s;
    }
}

// exclusive scan of tiles[0, nt) in place, the total to *count
__global__ __launch_bounds__(kScanThreads) void cloud_scan(int *__restrict__ tiles, int nt, int *__restrict__ count) {
    __shared__ int ws[kScanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int b = 0; b < nt; b += kScanThreads) {
        const int i = b + tid;
        const int v = i < nt ? tiles[i] : 0;
        int inc = v;  // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
            const int s = ws[w];
            pre += w < wave ? s : 0;
            tot += s;
        }
        if (i < nt) tiles[i] = carry + pre + inc - v;
        carry += tot;
        __syncthreads();  // the next chunk rewrites ws
    }
    if (tid == 0) *count = carry;
}

__global__ __launch_bounds__(kCThreads) void cloud_scatter(CloudArgs a, const int *__restrict__ tiles,
                                                           const uint8_t *__restrict__ color, int64_t cpitch, int ch,
                                                           float *__restrict__ pts, uint8_t *__restrict__ cols,
                                                           int *__restrict__ idx, int64_t cap) {
    __shared__ int wc[kCRounds * kCWaves];
#if DSX_CLOUD_STAGED
    __shared__ float sp[3 * kCT];
    __shared__ __attribute__((aligned(4))) uint8_t sc[3 * kCT + 4];
    __shared__ int si[kCT];
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t base = blockIdx.x * (uint32_t)kCT;
    const int64_t off = tiles[blockIdx.x];
    float d[kCRounds];
    unsigned long long m[kCRounds];
#pragma unroll
    for (int r = 0; r < kCRounds; ++r) {
        const uint32_t p = base + r * kCThreads + tid;
        bool v = false;
        d[r] = 0.0f;
        if (p < a.npix) {
            uint32_t x, y;
            float z;
            d[r] = cloud_load(a, p, x, y);
            v = cloud_z(a, d[r], z);
        }
        m[r] = __ballot(v);
        if (lane == 0) wc[r * kCWaves + wave] = __popcll(m[r]);
    }
    __syncthreads();
    int first[kCRounds] = {}, n = 0;  // points of the tile before this wave's of round r; the tile's count
#pragma unroll
    for (int r = 0; r < kCRounds; ++r) {
#pragma unroll
        for (int w = 0; w < kCWaves; ++w) {
            if (w == wave) first[r] = n;
            n += wc[r * kCWaves + w];
        }
    }
    // cap - off points of this tile have room (<= 0: none)
    const int nw = (int)max((int64_t)0, min((int64_t)n, cap - off));
#if DSX_CLOUD_STAGED
    // the colour bytes sit in LDS at their global range's misalignment, so aligned dwords match
    const int mis = cols ? (int)((reinterpret_cast<uintptr_t>(cols) + 3 * (uintptr_t)off) & 3u) : 0;
#endif
#pragma unroll
    for (int r = 0; r < kCRounds; ++r) {
        if (!((m[r] >> lane) & 1ull)) continue;
        const int rank = first[r] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m[r] >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)m[r], 0u));
        if (rank >= nw) continue;
        const uint32_t p = base + r * kCThreads + tid;
        const uint32_t y = p / a.W, x = p - y * a.W;
        float X, Y, Z;
        cloud_z(a, d[r], Z);
        cloud_xy(a, x, y, Z, X, Y);
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (cols) {
            const uint8_t *cp = color + (int64_t)y * cpitch + ((int64_t)a.x0 + x) * ch;
            if (ch == 3) c0 = cp[2], c1 = cp[1], c2 = cp[0];  // BGR -> RGB
            else c0 = c1 = c2 = cp[0];
        }
#if !DSX_CLOUD_STAGED
        const int64_t o = off + rank;
        pts[3 * o] = X;
        pts[3 * o + 1] = Y;
        pts[3 * o + 2] = Z;
        if (cols) cols[3 * o] = c0, cols[3 * o + 1] = c1, cols[3 * o + 2] = c2;
        if (idx) idx[o] = (int)p;
#else
        sp[3 * rank] = X;
        sp[3 * rank + 1] = Y;
        sp[3 * rank + 2] = Z;
        if (cols) sc[mis + 3 * rank] = c0, sc[mis + 3 * rank + 1] = c1, sc[mis + 3 * rank + 2] = c2;
        if (idx) si[rank] = (int)p;
#endif
    }
#if DSX_CLOUD_STAGED
    __syncthreads();
    float *po = pts + 3 * off;
    for (int i = tid; i < 3 * nw; i += kCThreads) po[i] = sp[i];
    if (idx) {
        int *io = idx + off;
        for (int i = tid; i < nw; i += kCThreads) io[i] = si[i];
    }
    if (cols) {
        // bytes [mis, mis + 3 nw) of the dword-aligned range that starts at cols + 3 off - mis
        uint8_t *co = cols + 3 * off - mis;
        const int end = mis + 3 * nw;
        for (int j = tid; 4 * j < end; j += kCThreads) {
            const int b = 4 * j;
            if (b >= mis && b + 4 <= end) {
                *reinterpret_cast<uint32_t *>(co + b) = *reinterpret_cast<const uint32_t *>(sc + b);
            } else {
                for (int k = max(b, mis); k < min(b + 4, end); ++k) co[k] = sc[k];
            }
        }
    }
#endif
}

int cloud_fail(const char *msg) { return dsx::set_error(DSX_EINVAL, msg); }

int check_cloud(const dsx_cloud *c) {
    if (!c) return cloud_fail("NULL cloud parameters");
    // in float32, as the device uses them: a focal length that rounds to 0 or inf there is refused too
    const float f = (float)c->focal_length, fB = (float)(c->focal_length * c->baseline);
    if (!(f > 0.0f) || !std::isfinite(f)) return cloud_fail("focal_length must be > 0 and finite");
    if (!std::isfinite(fB) || fB == 0.0f) return cloud_fail("baseline must be finite and != 0");
    if (!std::isfinite(c->cx) || !std::isfinite(c->cy)) return cloud_fail("the principal point must be finite");
    if (!std::isfinite(c->doffs) || !std::isfinite(c->eps)) return cloud_fail("doffs and eps must be finite");
    if (c->has_max_depth != 0 && c->has_max_depth != 1) return cloud_fail("has_max_depth must be 0 or 1");
    if (c->has_max_depth && !(c->max_depth > 0.0f)) return cloud_fail("max_depth must be > 0");
    if (c->x0 < 0) return cloud_fail("x0 must be >= 0");
    return DSX_OK;
}

// shape, pitch and parameters shared by both device calls; H, W >= 0 here
int cloud_args(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, const dsx_cloud *c, CloudArgs &a) {
    if (int rc = check_cloud(c)) return rc;
    if (H < 0 || W < 0) return cloud_fail("bad shape");
    if (H == 0 || W == 0) return DSX_OK;
    if (!d_disp) return cloud_fail("d_disp is NULL");
    if (in_pitch < W) return cloud_fail("bad pitch");
    if ((int64_t)H * W > 0x7FFFFFFF || (int64_t)c->x0 + W > 0x7FFFFFFF) return cloud_fail("image too large");
    a.disp = static_cast<const float *>(d_disp);
    a.pitch = in_pitch;
    a.W = (uint32_t)W;
    a.npix = (uint32_t)H * (uint32_t)W;
    a.fB = (float)(c->focal_length * c->baseline);  // the depth map's own constant (dsx_api.hip post_full_args)
    a.f = (float)c->focal_length;
    a.cx = c->cx, a.cy = c->cy, a.doffs = c->doffs, a.eps = c->eps, a.max_depth = c->max_depth;
    a.has_max = c->has_max_depth;
    a.x0 = c->x0;
    return DSX_OK;
}

int hip_fail(const char *what, hipError_t e) {
    return dsx::set_error(e == hipErrorOutOfMemory ? DSX_ENOMEM : DSX_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int dsx_check_cloud(const dsx_cloud *c) {
    dsx::set_error(DSX_OK, "");
    return check_cloud(c);
}

int dsx_reproject_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, const dsx_cloud *c, void *d_xyz,
                         void *hip_stream) {
    dsx::set_error(DSX_OK, "");
    CloudArgs a{};
    if (int rc = cloud_args(d_disp, H, W, in_pitch, c, a)) return rc;
    if (H == 0 || W == 0) return DSX_OK;
    if (!d_xyz) return cloud_fail("d_xyz is NULL");
    const uint32_t blocks = (a.npix + kCThreads - 1) / kCThreads;
    hipLaunchKernelGGL(cloud_reproject, dim3(blocks), dim3(kCThreads), 0, static_cast<hipStream_t>(hip_stream), a,
                       static_cast<float *>(d_xyz));
    if (hipError_t e = hipGetLastError()) return hip_fail("cloud_reproject", e);
    return DSX_OK;
}

int64_t dsx_point_cloud_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > 0x7FFFFFFF) return 0;
    return (((int64_t)H * W + kCT - 1) / kCT) * (int64_t)sizeof(int);
}

int dsx_point_cloud_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, const dsx_cloud *c,
                           const void *d_color, int64_t color_pitch_bytes, int32_t channels, void *d_points,
                           void *d_colors, void *d_index, int64_t cap, void *d_count, void *d_workspace,
                           int64_t workspace_bytes, void *hip_stream) {
    dsx::set_error(DSX_OK, "");
    CloudArgs a{};
    if (int rc = cloud_args(d_disp, H, W, in_pitch, c, a)) return rc;
    if (!d_count) return cloud_fail("d_count is NULL");
    if (cap < 0) return cloud_fail("cap must be >= 0");
    if (channels != 0 && channels != 1 && channels != 3) return cloud_fail("channels must be 0, 1 or 3");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (H == 0 || W == 0) {
        if (hipError_t e = hipMemsetAsync(d_count, 0, sizeof(int), st)) return hip_fail("hipMemsetAsync", e);
        return DSX_OK;
    }
    if (cap > 0 && !d_points) return cloud_fail("d_points is NULL");
    if (d_colors) {
        if (channels == 0 || !d_color) return cloud_fail("d_colors needs a colour image (d_color, channels 1 or 3)");
        if (color_pitch_bytes < ((int64_t)c->x0 + W) * channels) return cloud_fail("bad colour pitch");
    }
    if (!d_workspace || workspace_bytes < dsx_point_cloud_workspace_bytes(H, W))
        return cloud_fail("workspace too small (dsx_point_cloud_workspace_bytes)");
    const int nt = (int)((a.npix + (uint32_t)kCT - 1) / (uint32_t)kCT);
    int *tiles = static_cast<int *>(d_workspace);
    hipLaunchKernelGGL(cloud_count, dim3(nt), dim3(kCThreads), 0, st, a, tiles);
    hipLaunchKernelGGL(cloud_scan, dim3(1), dim3(kScanThreads), 0, st, tiles, nt, static_cast<int *>(d_count));
    hipLaunchKernelGGL(cloud_scatter, dim3(nt), dim3(kCThreads), 0, st, a, tiles, static_cast<const uint8_t *>(d_color),
                       color_pitch_bytes, (int)channels, static_cast<float *>(d_points), static_cast<uint8_t *>(d_colors),
                       static_cast<int *>(d_index), cap);
    if (hipError_t e = hipGetLastError()) return hip_fail("point cloud launches", e);
    return DSX_OK;
}

}  // extern "C"
