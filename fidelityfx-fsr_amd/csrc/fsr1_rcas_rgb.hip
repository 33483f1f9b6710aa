// RCAS on packed 3-channel RGB images (FSR1_FORMAT_RGB16F / RGB32F / RGB8_UNORM): the strip kernel of fsr1_rcas_planar.hip on
// interleaved elements, no LDS, no barrier.
//
// RCAS is the pass that is bound by its bytes: three elements per pixel move 6 / 12 / 3 B where the RGBA
// formats move 8 / 16 / 4, and the caller's pad to four channels and slice back to three — a full-image copy each — are gone.
//   * a wave owns a 256-column strip and walks it row by row — downwards in even strip rows, upwards in odd ones, so that vertically
//     adjacent strips meet at the rows they share; a lane owns FOUR adjacent pixels: twelve consecutive elements R0 G0 B0 .. B3, which
//     are exactly three accesses of four elements (4 / 8 / 16 bytes), aligned wherever the row is (RgbGroup, fsr1_device_rgb.hpp).
//     Per row a lane issues three such loads and three stores and unpacks in registers: 8-bit codes stay packed in three dwords
//     while in flight, a row is decoded once, as it becomes `next` (one v_cvt_f32_ubyteN per element), and the twelve results are
//     encoded and merged into three dwords before the store;
//   * of the horizontal taps of a lane's four pixels, six are its own registers and two are the facing pixels of the adjacent lanes,
//     fetched in fp32 by DPP wave shifts: six moves per four pixels;
//   * lanes 0 and 63 load the apron pixel, three elements, which the DPP move leaves in place for exactly those lanes;
//   * rows live in a register ring: prev / cur / next as fp32, raw rows in flight ahead of the arithmetic (2 deep for a launch short
//     of waves, 4 for batches; 8-bit codes: always 4, three registers a row);
//   * the per-pixel function is rcas_pixel<EXACT> with the interleaved kernel's operand order (b above, h below whichever way the
//     strip walks): every value is the one the RGBA kernel stores for the same pixels with alpha 1;
//   * taps outside the image are 0; strips wholly inside the image run a branch-free body, the image's first / last wave-column the
//     same body with its apron texel replaced, everything else (a width that is no multiple of four among it) a fully predicated
//     one, whose last lane moves its partial group element by element;
//   * WIDE = false — base, pitch or frame stride not a multiple of the four-element access (a tightly packed odd width) — moves
//     every element by itself: no access is ever wider than its alignment.
#include "fsr1_device.h"
#include "fsr1_device_rgb.hpp"

namespace fsr1 {

constexpr int kRcasRgbWaveCols = 256;  // columns per wave (four per lane)
constexpr int kRcasRgbWaves = 2;       // waves per workgroup, side by side
constexpr int kRcasRgbThreads = 64 * kRcasRgbWaves;
constexpr int kRcasRgbCols = kRcasRgbWaveCols * kRcasRgbWaves;

template <int CTRL>
__device__ __forceinline__ rgb_t rgb_neighbour(rgb_t keep, rgb_t v) {
  return rgb_t{dpp_f32<CTRL>(keep.r, v.r), dpp_f32<CTRL>(keep.g, v.g), dpp_f32<CTRL>(keep.b, v.b)};
}

template <int FMT, bool EXACT, bool OPTS, bool WIDE, bool INTERIOR, int RING, bool XEDGE = false, bool UP = false>
__device__ __forceinline__ void rcas_rgb_strip(const RcasArgs& a, int frame, int x0, int y0, int lane) {
  typedef Rgb3<FMT> P;
  typedef typename P::E elem_t;
  typedef typename P::V4 quad_t;
  constexpr uint32_t kPixel = 3 * sizeof(elem_t);
  const uint32_t flags = OPTS ? a.flags : 0u;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  const int W = a.in.width, H = a.in.height;
  const int col = x0 + 4 * lane;
  const bool ok[4] = {INTERIOR || col < W, INTERIOR || col + 1 < W, INTERIOR || col + 2 < W, INTERIOR || col + 3 < W};
  const bool edge = lane == 0 || lane == 63;
  // apron pixel of lanes 0 / 63; the other lanes point at their own pixel, so that the interior body loads unconditionally
  const int hcol = lane == 0 ? x0 - 1 : (lane == 63 ? x0 + kRcasRgbWaveCols : col);
  const bool halo_ok = edge && ((INTERIOR && !XEDGE) || (hcol >= 0 && hcol < W));
  const bool halo_out = XEDGE && edge && !halo_ok;  // (an outside apron pixel is never addressed: its lane re-reads column 0 / W - 1)
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;
  const uint32_t off = (uint32_t)col * kPixel, hoff = (uint32_t)min(max(hcol, 0), W - 1) * kPixel;
  auto zext = [](uint32_t o) { asm("" : "+v"(o)); return (size_t)o; };  // (keeps the lane offset next to its use: fsr1_rcas_kernel.h)

  const int rows = a.rows;
  static_assert(!UP || INTERIOR, "only strips that store every row walk up");
  auto row_y = [&](int k) { return UP ? y0 + rows - 1 - k : y0 + k; };  // k-th row of the walk, k = -1 .. rows
  struct row_t { RgbGroup<FMT> g; elem_t halo[3]; };
  const quad_t zero4 = P::make4((elem_t)0, (elem_t)0, (elem_t)0, (elem_t)0);
  auto load = [&](int y, row_t& r) {
    const bool row_in = INTERIOR || (y >= 0 && y < H);  // wave-uniform
    const char* const src = in_frame + (long long)y * a.in.pitch;  // scalar (an outside row is never dereferenced)
    const elem_t* const e = reinterpret_cast<const elem_t*>(src + zext(off));
    const elem_t* const he = reinterpret_cast<const elem_t*>(src + zext(hoff));
    if (INTERIOR) {
      if constexpr (WIDE) {
#pragma unroll
        for (int j = 0; j < 3; ++j) r.g.w[j] = reinterpret_cast<const quad_t*>(e)[j];
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) r.g.w[j] = P::make4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) r.halo[c] = he[c];
      if constexpr (XEDGE) {
        if (halo_out) r.halo[0] = r.halo[1] = r.halo[2] = (elem_t)0;
      }
    } else {
      r.g.w[0] = r.g.w[1] = r.g.w[2] = zero4;
      r.halo[0] = r.halo[1] = r.halo[2] = (elem_t)0;
      if (row_in) {
        if (WIDE && ok[3]) {
#pragma unroll
          for (int j = 0; j < 3; ++j) r.g.w[j] = reinterpret_cast<const quad_t*>(e)[j];
        } else {
#define FSR1_RCASR_PX(I) if (ok[I]) { r.g.template put<3 * I>(e[3 * I]); r.g.template put<3 * I + 1>(e[3 * I + 1]); r.g.template put<3 * I + 2>(e[3 * I + 2]); }
          FSR1_RCASR_PX(0) FSR1_RCASR_PX(1) FSR1_RCASR_PX(2) FSR1_RCASR_PX(3)
#undef FSR1_RCASR_PX
        }
        if (halo_ok) {
#pragma unroll
          for (int c = 0; c < 3; ++c) r.halo[c] = he[c];
        }
      }
    }
  };
  struct px4_t { rgb_t v[4]; };
  auto rgb4 = [](const row_t& r) {
    return px4_t{{r.g.template pixel<0>(), r.g.template pixel<1>(), r.g.template pixel<2>(), r.g.template pixel<3>()}};
  };
  // ring of raw rows in registers, loads kAhead rows ahead of the arithmetic; the row loop is unrolled by the ring (static indices)
  constexpr int kRing = RING, kAhead = kRing - 1;  // divides every strip height the launcher picks (multiples of 8)
  row_t q[kRing];
  px4_t prev, cur;
  {
    row_t q_prev;
    load(row_y(-1), q_prev);
#pragma unroll
    for (int k = 0; k < kAhead; ++k) load(row_y(k), q[k]);
    prev = rgb4(q_prev);
    cur = rgb4(q[0]);
  }
  const float sharp = as_f32(a.con[0]);

#pragma unroll 1
  for (int r0 = 0; r0 < rows; r0 += kRing) {
#pragma unroll
    for (int k = 0; k < kRing; ++k) {
      const int y = row_y(r0 + k);
      load(row_y(min(r0 + k + kAhead, rows)), q[(k + kAhead) % kRing]);  // past the end: re-reads the last row (harmless, branch-free)
      const row_t& c = q[k];
      const px4_t next = rgb4(q[(k + 1) % kRing]);
      const rgb_t hal = {P::load(c.halo[0]), P::load(c.halo[1]), P::load(c.halo[2])};
      // pixel 0's left tap = the left lane's pixel 3, pixel 3's right tap = the right lane's pixel 0; lanes 0 / 63 keep their apron pixel
      const rgb_t d0 = rgb_neighbour<kDppWaveShr1>(hal, cur.v[3]), f3 = rgb_neighbour<kDppWaveShl1>(hal, cur.v[0]);
      const px4_t& above = UP ? next : prev;  // b is the tap above, h the one below (ffx_fsr1.h:697-707), whichever way the strip walks
      const px4_t& below = UP ? prev : next;
      const rgb_t o[4] = {rcas_pixel<EXACT>(above.v[0], d0, cur.v[0], cur.v[1], below.v[0], sharp, flags),
                          rcas_pixel<EXACT>(above.v[1], cur.v[0], cur.v[1], cur.v[2], below.v[1], sharp, flags),
                          rcas_pixel<EXACT>(above.v[2], cur.v[1], cur.v[2], cur.v[3], below.v[2], sharp, flags),
                          rcas_pixel<EXACT>(above.v[3], cur.v[2], cur.v[3], f3, below.v[3], sharp, flags)};
      if (INTERIOR || y < H) {
        char* const dst = out_frame + (long long)y * a.out.pitch + zext(off);
        if (WIDE && ok[3]) {  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
          store_out<sizeof(quad_t)>(dst, P::store4(o[0].r, o[0].g, o[0].b, o[1].r), stream);
          store_out<sizeof(quad_t)>(dst + sizeof(quad_t), P::store4(o[1].g, o[1].b, o[2].r, o[2].g), stream);
          store_out<sizeof(quad_t)>(dst + 2 * sizeof(quad_t), P::store4(o[2].b, o[3].r, o[3].g, o[3].b), stream);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (!ok[i]) continue;
            store_out<sizeof(elem_t)>(dst + i * kPixel, P::store(o[i].r), stream);
            store_out<sizeof(elem_t)>(dst + i * kPixel + sizeof(elem_t), P::store(o[i].g), stream);
            store_out<sizeof(elem_t)>(dst + i * kPixel + 2 * sizeof(elem_t), P::store(o[i].b), stream);
          }
        }
      }
      prev = cur;
      cur = next;
    }
  }
}

// OPTS = false: the plain pass (no denoise / HDR square), flags compiled out.  RING: raw rows in flight per lane.
template <int FMT, bool EXACT, bool OPTS, bool WIDE, int RING>
__global__ void __launch_bounds__(kRcasRgbThreads) rcas_rgb_kernel(const RcasArgs a) {
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = tx * kRcasRgbCols + wave * kRcasRgbWaveCols, y0 = ty * a.rows;
  if (x0 >= a.in.width) return;  // whole wave outside (no barriers in this kernel)
  const bool interior_y = y0 >= 1 && y0 + a.rows + 1 <= a.in.height;  // every row the strip reads and stores is inside
  const bool inside_x = x0 + kRcasRgbWaveCols <= a.in.width;
  const bool interior = interior_y && x0 >= 1 && x0 + kRcasRgbWaveCols + 1 <= a.in.width;
  const bool up = (ty & 1) != 0;
  if (interior && up) rcas_rgb_strip<FMT, EXACT, OPTS, WIDE, true, RING, false, true>(a, frame, x0, y0, lane);
  else if (interior) rcas_rgb_strip<FMT, EXACT, OPTS, WIDE, true, RING>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x && up) rcas_rgb_strip<FMT, EXACT, OPTS, WIDE, true, RING, true, true>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x) rcas_rgb_strip<FMT, EXACT, OPTS, WIDE, true, RING, true>(a, frame, x0, y0, lane);
  else rcas_rgb_strip<FMT, EXACT, OPTS, WIDE, false, RING>(a, frame, x0, y0, lane);
}

// Strip height by fsr1_rcas.hip's rule on this kernel's 256-column waves (as rcas_planar_geometry): 16 rows unless that leaves fewer
// than four waves per SIMD (and the launch does not run beside other frames' launches), then 8.
void rcas_rgb_geometry(int width, int height, int frames, bool overlapped, int* tiles_x, int* tiles_y, int* rows) {
  const int tx = (width + kRcasRgbCols - 1) / kRcasRgbCols;
  int r = 16;
  if (!overlapped && (long long)tx * ((height + r - 1) / r) * frames * kRcasRgbWaves < 4LL * 4 * 256) r = 8;
  *rows = r;
  *tiles_x = tx;
  *tiles_y = (height + r - 1) / r;
}

// RING by the launch, the planar kernel's rule (a row in flight costs a lane the same registers there and here): the shallow ring
// when the launch is short of waves, fewer than 6 per SIMD in 16-row strips; 8-bit codes keep four rows in flight whatever the launch.
template <int FMT, bool EXACT, bool OPTS, bool WIDE>
static void rcas_rgb_launch_one(const RcasArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasRgbThreads);
  if constexpr (FMT != FSR1_FORMAT_RGB8_UNORM) {
    if ((long long)a.tiles_x * ((a.in.height + 15) / 16) * a.frames * kRcasRgbWaves < 6LL * 4 * 256) {
      hipLaunchKernelGGL((rcas_rgb_kernel<FMT, EXACT, OPTS, WIDE, 2>), grid, block, 0, stream, a);
      return;
    }
  }
  hipLaunchKernelGGL((rcas_rgb_kernel<FMT, EXACT, OPTS, WIDE, 4>), grid, block, 0, stream, a);
}

// wide: the four-element accesses (the host has checked both images' base, pitch and frame stride against them).
hipError_t rcas_rgb_launch(const RcasArgs& a, int fmt, bool exact, bool wide, hipStream_t stream) {
  const bool opts = (a.flags & (FSR1_FLAG_RCAS_DENOISE | FSR1_FLAG_HDR_SQUARE)) != 0;
#define FSR1_RCASR(F, E, O, V) rcas_rgb_launch_one<F, E, O, V>(a, stream)
#define FSR1_RCASR_V(F, E, O) do { if (wide) FSR1_RCASR(F, E, O, true); else FSR1_RCASR(F, E, O, false); } while (0)
#define FSR1_RCASR_O(F, E) do { if (opts) FSR1_RCASR_V(F, E, true); else FSR1_RCASR_V(F, E, false); } while (0)
#define FSR1_RCASR_E(F) do { if (exact) FSR1_RCASR_O(F, true); else FSR1_RCASR_O(F, false); } while (0)
  switch (fmt) {
    case FSR1_FORMAT_RGB16F: FSR1_RCASR_E(FSR1_FORMAT_RGB16F); break;
    case FSR1_FORMAT_RGB32F: FSR1_RCASR_E(FSR1_FORMAT_RGB32F); break;
    case FSR1_FORMAT_RGB8_UNORM: FSR1_RCASR_E(FSR1_FORMAT_RGB8_UNORM); break;
    default: return hipErrorInvalidValue;
  }
#undef FSR1_RCASR_E
#undef FSR1_RCASR_O
#undef FSR1_RCASR_V
#undef FSR1_RCASR
  return hipGetLastError();
}

}  // namespace fsr1
