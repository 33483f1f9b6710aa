// Stand-alone colour pass: out = stages(in), stages = FsrSrtmF -> FsrLfgaF -> FsrSrtmInvF -> FsrTepdC8F|C10F
// (ffx-fsr/ffx_fsr1.h:986-1199; the reference leaves the pass itself to the integration, e.g.
// sample/src/DX12/FSR_Tonemapping.hlsl:87).
//
// Pure streaming work, HBM bound (in + out bytes per pixel, ~60 VALU instructions with every stage on): a wave
// owns a 128-column x 8-row block, a lane two adjacent pixels (one 16-byte access per row for RGBA16F), all eight
// row loads are issued before the first use; the four waves of a workgroup stack vertically (128 x 32 tile).
// The noise tile (a few KiB) stays in L2.
#include "fsr1_device_color.hpp"
#include "fsr1_device_half.hpp"
#include "fsr1_device.h"

namespace fsr1 {

constexpr int kColorCols = 128, kColorRowsPerWave = 8, kColorRows = 4 * kColorRowsPerWave;

template <int FIN, int FOUT, bool EXACT>
__global__ void __launch_bounds__(kThreads) color_kernel(const ColorPassArgs a) {
  typedef typename Pixel<FIN>::T in_t;
  typedef typename Pixel<FOUT>::T out_t;
  struct __attribute__((aligned(4))) in2_t { char bytes[2 * sizeof(in_t)]; };    // two adjacent texels, one access
  struct __attribute__((aligned(4))) out2_t { char bytes[2 * sizeof(out_t)]; };
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tx * kColorCols + 2 * lane, y0 = ty * kColorRows + wave * kColorRowsPerWave;
  const int W = a.in.width, H = a.in.height;
  if (x >= W || y0 >= H) return;
  const bool pair = x + 1 < W;
  const char* src = a.in.base + (long long)frame * a.in.frame_stride + (size_t)x * sizeof(in_t);
  char* dst = a.out.base + (long long)frame * a.out.frame_stride + (size_t)x * sizeof(out_t);

  in_t q[kColorRowsPerWave][2];
#pragma unroll
  for (int r = 0; r < kColorRowsPerWave; ++r) {
    const int y = min(y0 + r, H - 1);
    const char* p = src + (long long)y * a.in.pitch;
    if (pair) {
      const in2_t v = *reinterpret_cast<const in2_t*>(p);
      __builtin_memcpy(&q[r][0], v.bytes, sizeof(in_t));
      __builtin_memcpy(&q[r][1], v.bytes + sizeof(in_t), sizeof(in_t));
    } else {
      q[r][0] = *reinterpret_cast<const in_t*>(p);
      q[r][1] = q[r][0];
    }
  }
#pragma unroll
  for (int r = 0; r < kColorRowsPerWave; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    out_t o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float4_t c = Pixel<FIN>::load(q[r][i]);
      c = color_prologue<EXACT>(a.color, c);
      c = color_epilogue<EXACT>(a.color, (uint32_t)(x + i), (uint32_t)y, c);
      o[i] = Pixel<FOUT>::store(c.x, c.y, c.z, c.w);
    }
    char* p = dst + (long long)y * a.out.pitch;
    if (pair) {
      out2_t v;
      __builtin_memcpy(v.bytes, &o[0], sizeof(out_t));
      __builtin_memcpy(v.bytes + sizeof(out_t), &o[1], sizeof(out_t));
      *reinterpret_cast<out2_t*>(p) = v;
    } else {
      *reinterpret_cast<out_t*>(p) = o[0];
    }
  }
}

// ---- packed binary16 arithmetic (parity class "H"): color_prologue_h2 / color_epilogue_h2 of fsr1_device_color_half.hpp — the
//      reference's Hx2 stages, a lane's adjacent pixels in the two halves of every AH2, bit-identical to the CPU-evaluated H path.
//      Loads and stores follow TexelH (fsr1_device_half.hpp), alpha passes through it unchanged. ----
// RGBA16F in and out: two pixels per lane, one 16-byte access each way per row.
__global__ void __launch_bounds__(kThreads) color_h_kernel(const ColorPassArgs a) {
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tx * kColorCols + 2 * lane, y0 = ty * kColorRows + wave * kColorRowsPerWave;
  const int W = a.in.width, H = a.in.height;
  if (x >= W || y0 >= H) return;
  const bool pair = x + 1 < W;
  const char* src = a.in.base + (long long)frame * a.in.frame_stride + (size_t)x * sizeof(half4_t);
  char* dst = a.out.base + (long long)frame * a.out.frame_stride + (size_t)x * sizeof(half4_t);
  struct __attribute__((aligned(8))) px2_t { half4_t p[2]; };
#pragma unroll 1
  for (int r = 0; r < kColorRowsPerWave; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    px2_t q;
    if (pair) q = *reinterpret_cast<const px2_t*>(src + (long long)y * a.in.pitch);
    else { q.p[0] = *reinterpret_cast<const half4_t*>(src + (long long)y * a.in.pitch); q.p[1] = q.p[0]; }
    rgbh2_t c = {c_h2(q.p[0].x, q.p[1].x), c_h2(q.p[0].y, q.p[1].y), c_h2(q.p[0].z, q.p[1].z)};
    color_prologue_h2(a.color, c);
    color_epilogue_h2(a.color, (uint32_t)x, (uint32_t)x + 1u, (uint32_t)y, c);
    px2_t o;
    o.p[0] = half4_t{c.r.x, c.g.x, c.b.x, q.p[0].w};
    o.p[1] = half4_t{c.r.y, c.g.y, c.b.y, q.p[1].w};
    char* p = dst + (long long)y * a.out.pitch;
    if (pair) *reinterpret_cast<px2_t*>(p) = o;
    else *reinterpret_cast<half4_t*>(p) = o.p[0];
  }
}

// A 32 bpp UNORM format on either side: FOUR adjacent pixels per lane, so that the 4-byte side moves as one 16-byte access per
// lane-row (an RGBA16F side as two, 32 contiguous bytes) — the access width this chip moves at full rate (fsr1_rcas_h.hip).  A wave
// covers 256 columns x 8 rows, the four waves of a workgroup stack vertically (256 x 32 tile).  A lane reads its four texels before it
// writes them, so the pass runs in place when the formats match.
constexpr int kColorH4Cols = 4 * 64;

// n (1 .. 4) adjacent texels of a row; rows are only texel-aligned.  A ragged right edge goes texel by texel.
template <int FMT>
struct QuadH {
  typedef typename TexelH<FMT>::T tex_t;
  struct __attribute__((aligned(sizeof(tex_t) < 8 ? 4 : 8))) T { tex_t v[4]; };
  static __device__ __forceinline__ void load(const char* p, int n, half4_t t[4]) {
    T q;
    if (n == 4) {
      q = *reinterpret_cast<const T*>(p);
    } else {
      const tex_t* const px = reinterpret_cast<const tex_t*>(p);
      q.v[0] = px[0];
      q.v[1] = n > 1 ? px[1] : q.v[0];
      q.v[2] = n > 2 ? px[2] : q.v[0];
      q.v[3] = q.v[0];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = TexelH<FMT>::load(q.v[i]);
  }
  static __device__ __forceinline__ void store(char* p, int n, const half4_t t[4]) {
    T q;
#pragma unroll
    for (int i = 0; i < 4; ++i) q.v[i] = TexelH<FMT>::store(t[i]);
    if (n == 4) {
      *reinterpret_cast<T*>(p) = q;
    } else {
      tex_t* const px = reinterpret_cast<tex_t*>(p);
      px[0] = q.v[0];
      if (n > 1) px[1] = q.v[1];
      if (n > 2) px[2] = q.v[2];
    }
  }
};

template <int FIN, int FOUT>
__global__ void __launch_bounds__(kThreads) color_h4_kernel(const ColorPassArgs a) {
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tx * kColorH4Cols + 4 * lane, y0 = ty * kColorRows + wave * kColorRowsPerWave;
  const int W = a.in.width, H = a.in.height;
  if (x >= W || y0 >= H) return;
  const int n = min(W - x, 4);  // this lane's pixels inside the image
  const char* src = a.in.base + (long long)frame * a.in.frame_stride + (size_t)x * sizeof(typename TexelH<FIN>::T);
  char* dst = a.out.base + (long long)frame * a.out.frame_stride + (size_t)x * sizeof(typename TexelH<FOUT>::T);
#pragma unroll 1
  for (int r = 0; r < kColorRowsPerWave; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    half4_t q[4];
    QuadH<FIN>::load(src + (long long)y * a.in.pitch, n, q);
    rgbh2_t lo = {c_h2(q[0].x, q[1].x), c_h2(q[0].y, q[1].y), c_h2(q[0].z, q[1].z)};
    rgbh2_t hi = {c_h2(q[2].x, q[3].x), c_h2(q[2].y, q[3].y), c_h2(q[2].z, q[3].z)};
    color_prologue_h2(a.color, lo);
    color_prologue_h2(a.color, hi);
    // (the noise tile wraps, so the positions of a ragged lane's missing pixels are fetched harmlessly)
    color_epilogue_h2(a.color, (uint32_t)x, (uint32_t)x + 1u, (uint32_t)y, lo);
    color_epilogue_h2(a.color, (uint32_t)x + 2u, (uint32_t)x + 3u, (uint32_t)y, hi);
    const half4_t o[4] = {half4_t{lo.r.x, lo.g.x, lo.b.x, q[0].w}, half4_t{lo.r.y, lo.g.y, lo.b.y, q[1].w},
                          half4_t{hi.r.x, hi.g.x, hi.b.x, q[2].w}, half4_t{hi.r.y, hi.g.y, hi.b.y, q[3].w}};
    QuadH<FOUT>::store(dst + (long long)y * a.out.pitch, n, o);
  }
}

static bool color_h_two_pixel(int fin, int fout) { return fin == FSR1_FORMAT_RGBA16F && fout == FSR1_FORMAT_RGBA16F; }

void color_h_geometry(int fin, int fout, int width, int height, int* tiles_x, int* tiles_y) {
  const int cols = color_h_two_pixel(fin, fout) ? kColorCols : kColorH4Cols;
  *tiles_x = (width + cols - 1) / cols;
  *tiles_y = (height + kColorRows - 1) / kColorRows;
}

hipError_t color_h_launch(const ColorPassArgs& a, int fin, int fout, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kThreads);
  constexpr int F16 = FSR1_FORMAT_RGBA16F, U8 = FSR1_FORMAT_RGBA8_UNORM, U10 = FSR1_FORMAT_R10G10B10A2_UNORM;
#define FSR1_COLOR_H4(I, O) hipLaunchKernelGGL((color_h4_kernel<I, O>), grid, block, 0, stream, a)
  if (color_h_two_pixel(fin, fout)) hipLaunchKernelGGL(color_h_kernel, grid, block, 0, stream, a);
  else if (fin == F16 && fout == U8) FSR1_COLOR_H4(F16, U8);
  else if (fin == F16 && fout == U10) FSR1_COLOR_H4(F16, U10);
  else if (fin == U8 && fout == F16) FSR1_COLOR_H4(U8, F16);
  else if (fin == U8 && fout == U8) FSR1_COLOR_H4(U8, U8);
  else if (fin == U8 && fout == U10) FSR1_COLOR_H4(U8, U10);
  else if (fin == U10 && fout == F16) FSR1_COLOR_H4(U10, F16);
  else if (fin == U10 && fout == U8) FSR1_COLOR_H4(U10, U8);
  else if (fin == U10 && fout == U10) FSR1_COLOR_H4(U10, U10);
  else return hipErrorInvalidValue;
#undef FSR1_COLOR_H4
  return hipGetLastError();
}

void color_geometry(int width, int height, int* tiles_x, int* tiles_y) {
  *tiles_x = (width + kColorCols - 1) / kColorCols;
  *tiles_y = (height + kColorRows - 1) / kColorRows;
}

hipError_t color_launch(const ColorPassArgs& a, int fin, int fout, bool exact, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kThreads);
#define FSR1_COLOR(I, O, E) hipLaunchKernelGGL((color_kernel<I, O, E>), grid, block, 0, stream, a)
#define FSR1_COLOR_E(I, O) do { if (exact) FSR1_COLOR(I, O, true); else FSR1_COLOR(I, O, false); } while (0)
#define FSR1_COLOR_O(I)                                                                        \
  switch (fout) {                                                                              \
    case FSR1_FORMAT_RGBA16F: FSR1_COLOR_E(I, FSR1_FORMAT_RGBA16F); break;                     \
    case FSR1_FORMAT_RGBA32F: FSR1_COLOR_E(I, FSR1_FORMAT_RGBA32F); break;                     \
    case FSR1_FORMAT_RGBA8_UNORM: FSR1_COLOR_E(I, FSR1_FORMAT_RGBA8_UNORM); break;             \
    case FSR1_FORMAT_R10G10B10A2_UNORM: FSR1_COLOR_E(I, FSR1_FORMAT_R10G10B10A2_UNORM); break; \
    default: return hipErrorInvalidValue;                                                      \
  }
  switch (fin) {
    case FSR1_FORMAT_RGBA16F: FSR1_COLOR_O(FSR1_FORMAT_RGBA16F); break;
    case FSR1_FORMAT_RGBA32F: FSR1_COLOR_O(FSR1_FORMAT_RGBA32F); break;
    case FSR1_FORMAT_RGBA8_UNORM: FSR1_COLOR_O(FSR1_FORMAT_RGBA8_UNORM); break;
    case FSR1_FORMAT_R10G10B10A2_UNORM: FSR1_COLOR_O(FSR1_FORMAT_R10G10B10A2_UNORM); break;
    default: return hipErrorInvalidValue;
  }
#undef FSR1_COLOR_O
#undef FSR1_COLOR_E
#undef FSR1_COLOR
  return hipGetLastError();
}

}  // namespace fsr1
