// RCAS on planar RGB images (FSR1_FORMAT_RGB16F_PLANAR / RGB32F_PLANAR / RGB8_UNORM_PLANAR): a strip kernel of its own, no LDS, no barrier.
//
// RCAS is the pass that is bound by its bytes, and an interleaved RGBA16F pixel carries a quarter of them as
// an alpha that is read and written as 1: three planes move 12 B per pixel where RGBA16F moves 16.
//   * a wave owns a 256-column strip and walks it row by row — downwards in even strip rows, upwards in odd ones, so that vertically
//     adjacent strips meet at the rows they share (fsr1_rcas_kernel.h, UP); a lane owns FOUR adjacent columns: per row and plane one
//     8-byte (fp16) or 16-byte (fp32) load and one store of the same width; 8-bit planes: one DWORD each way, the raw rows stay in
//     flight as packed dwords (three registers a row), a row is decoded once, as it becomes `next`, and the four results of a plane
//     are encoded and merged before the store: 3 B in and 3 B out per pixel where RGBA8 moves 4 + 4;
//   * of the horizontal taps of a lane's four pixels, six are its own registers and two are the facing pixels of the adjacent lanes,
//     fetched in fp32 by DPP wave shifts: six moves per four pixels (the interleaved kernel: six per two);
//   * lanes 0 and 63 load the apron column, one element per plane, which the DPP move leaves in place for exactly those lanes;
//   * rows live in a register ring: prev / cur / next as fp32, raw rows in flight ahead of the arithmetic (2 deep for a launch short
//     of waves, 4 for batches; 8-bit planes: always 4);
//   * the per-pixel function is rcas_pixel<EXACT> with the interleaved kernel's operand order (b above, h below whichever way the
//     strip walks): every value is the one that kernel stores for the same pixels with alpha 1;
//   * taps outside the image are 0; strips wholly inside the image run a branch-free body, the image's first / last wave-column the
//     same body with its apron texel replaced, everything else a fully predicated one;
//   * WIDE = false — base, pitch, plane or frame stride not a multiple of the four-element access (a tightly packed odd width) —
//     moves every element by itself: no access is ever wider than its alignment.
#include "fsr1_device.h"
#include "fsr1_device_planar.hpp"

namespace fsr1 {

constexpr int kRcasPlanarWaveCols = 256;  // columns per wave (four per lane)
constexpr int kRcasPlanarWaves = 2;       // waves per workgroup, side by side
constexpr int kRcasPlanarThreads = 64 * kRcasPlanarWaves;
constexpr int kRcasPlanarCols = kRcasPlanarWaveCols * kRcasPlanarWaves;

template <int CTRL>
__device__ __forceinline__ rgb_t planar_neighbour(rgb_t keep, rgb_t v) {
  return rgb_t{dpp_f32<CTRL>(keep.r, v.r), dpp_f32<CTRL>(keep.g, v.g), dpp_f32<CTRL>(keep.b, v.b)};
}

template <int FMT, bool EXACT, bool OPTS, bool WIDE, bool INTERIOR, int RING, bool XEDGE = false, bool UP = false>
__device__ __forceinline__ void rcas_planar_strip(const RcasArgs& a, int frame, int x0, int y0, int lane) {
  typedef typename Plane<FMT>::E elem_t;
  typedef typename Plane<FMT>::V4 quad_t;
  const uint32_t flags = OPTS ? a.flags : 0u;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  const int W = a.in.width, H = a.in.height;
  const int col = x0 + 4 * lane;
  const bool ok[4] = {INTERIOR || col < W, INTERIOR || col + 1 < W, INTERIOR || col + 2 < W, INTERIOR || col + 3 < W};
  const bool edge = lane == 0 || lane == 63;
  // apron column of lanes 0 / 63; the other lanes point at their own column, so that the interior body loads unconditionally
  const int hcol = lane == 0 ? x0 - 1 : (lane == 63 ? x0 + kRcasPlanarWaveCols : col);
  const bool halo_ok = edge && ((INTERIOR && !XEDGE) || (hcol >= 0 && hcol < W));
  const bool halo_out = XEDGE && edge && !halo_ok;  // (an outside apron texel is never addressed: its lane re-reads column 0 / W - 1)
  const long long ips = plane_stride(a.in), ops = plane_stride(a.out);
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;
  const uint32_t off = (uint32_t)col * (uint32_t)sizeof(elem_t), hoff = (uint32_t)min(max(hcol, 0), W - 1) * (uint32_t)sizeof(elem_t);
  auto zext = [](uint32_t o) { asm("" : "+v"(o)); return (size_t)o; };  // (keeps the lane offset next to its use: fsr1_rcas_kernel.h)

  const int rows = a.rows;
  static_assert(!UP || INTERIOR, "only strips that store every row walk up");
  auto row_y = [&](int k) { return UP ? y0 + rows - 1 - k : y0 + k; };  // k-th row of the walk, k = -1 .. rows
  struct row_t { quad_t p[3]; elem_t halo[3]; };
  typedef Plane<FMT> P;
  const quad_t zero4 = P::make4((elem_t)0, (elem_t)0, (elem_t)0, (elem_t)0);
  auto load = [&](int y, row_t& r) {
    const bool row_in = INTERIOR || (y >= 0 && y < H);  // wave-uniform
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const char* const src = in_frame + c * ips + (long long)y * a.in.pitch;  // scalar
      if (INTERIOR) {
        if constexpr (WIDE) {
          r.p[c] = *reinterpret_cast<const quad_t*>(src + zext(off));
        } else {
          const elem_t* const e = reinterpret_cast<const elem_t*>(src + zext(off));
          r.p[c] = P::make4(e[0], e[1], e[2], e[3]);
        }
        r.halo[c] = *reinterpret_cast<const elem_t*>(src + zext(hoff));
        if constexpr (XEDGE) {
          if (halo_out) r.halo[c] = (elem_t)0;
        }
      } else {
        r.p[c] = zero4;
        r.halo[c] = (elem_t)0;
        if (row_in) {
          const elem_t* const e = reinterpret_cast<const elem_t*>(src + zext(off));
          if (WIDE && ok[3]) {
            r.p[c] = *reinterpret_cast<const quad_t*>(e);
          } else {
            if (ok[0]) P::template put<0>(r.p[c], e[0]);
            if (ok[1]) P::template put<1>(r.p[c], e[1]);
            if (ok[2]) P::template put<2>(r.p[c], e[2]);
            if (ok[3]) P::template put<3>(r.p[c], e[3]);
          }
          if (halo_ok) r.halo[c] = *reinterpret_cast<const elem_t*>(src + zext(hoff));
        }
      }
    }
  };
  struct px4_t { rgb_t v[4]; };
  auto rgb4 = [](const row_t& r) {
#define FSR1_RCASP_COL(I) rgb_t{P::load(P::template get<I>(r.p[0])), P::load(P::template get<I>(r.p[1])), P::load(P::template get<I>(r.p[2]))}
    return px4_t{{FSR1_RCASP_COL(0), FSR1_RCASP_COL(1), FSR1_RCASP_COL(2), FSR1_RCASP_COL(3)}};
#undef FSR1_RCASP_COL
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
      // pixel 0's left tap = the left lane's pixel 3, pixel 3's right tap = the right lane's pixel 0; lanes 0 / 63 keep their apron texel
      const rgb_t d0 = planar_neighbour<kDppWaveShr1>(hal, cur.v[3]), f3 = planar_neighbour<kDppWaveShl1>(hal, cur.v[0]);
      const px4_t& above = UP ? next : prev;  // b is the tap above, h the one below (ffx_fsr1.h:697-707), whichever way the strip walks
      const px4_t& below = UP ? prev : next;
      const rgb_t o0 = rcas_pixel<EXACT>(above.v[0], d0, cur.v[0], cur.v[1], below.v[0], sharp, flags);
      const rgb_t o1 = rcas_pixel<EXACT>(above.v[1], cur.v[0], cur.v[1], cur.v[2], below.v[1], sharp, flags);
      const rgb_t o2 = rcas_pixel<EXACT>(above.v[2], cur.v[1], cur.v[2], cur.v[3], below.v[2], sharp, flags);
      const rgb_t o3 = rcas_pixel<EXACT>(above.v[3], cur.v[2], cur.v[3], f3, below.v[3], sharp, flags);
      if (INTERIOR || y < H) {
        const float out[3][4] = {{o0.r, o1.r, o2.r, o3.r}, {o0.g, o1.g, o2.g, o3.g}, {o0.b, o1.b, o2.b, o3.b}};
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          char* const dst = out_frame + p * ops + (long long)y * a.out.pitch + zext(off);
          if (WIDE && ok[3]) {
            store_out<sizeof(quad_t)>(dst, P::store4(out[p][0], out[p][1], out[p][2], out[p][3]), stream);
          } else {
            if (ok[0]) store_out<sizeof(elem_t)>(dst, P::store(out[p][0]), stream);
            if (ok[1]) store_out<sizeof(elem_t)>(dst + sizeof(elem_t), P::store(out[p][1]), stream);
            if (ok[2]) store_out<sizeof(elem_t)>(dst + 2 * sizeof(elem_t), P::store(out[p][2]), stream);
            if (ok[3]) store_out<sizeof(elem_t)>(dst + 3 * sizeof(elem_t), P::store(out[p][3]), stream);
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
__global__ void __launch_bounds__(kRcasPlanarThreads) rcas_planar_kernel(const RcasArgs a) {
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = tx * kRcasPlanarCols + wave * kRcasPlanarWaveCols, y0 = ty * a.rows;
  if (x0 >= a.in.width) return;  // whole wave outside (no barriers in this kernel)
  const bool interior_y = y0 >= 1 && y0 + a.rows + 1 <= a.in.height;  // every row the strip reads and stores is inside
  const bool inside_x = x0 + kRcasPlanarWaveCols <= a.in.width;
  const bool interior = interior_y && x0 >= 1 && x0 + kRcasPlanarWaveCols + 1 <= a.in.width;
  const bool up = (ty & 1) != 0;
  if (interior && up) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING, false, true>(a, frame, x0, y0, lane);
  else if (interior) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x && up) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING, true, true>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING, true>(a, frame, x0, y0, lane);
  else rcas_planar_strip<FMT, EXACT, OPTS, WIDE, false, RING>(a, frame, x0, y0, lane);
}

// Strip height by fsr1_rcas.hip's rule on this kernel's 256-column waves: 16 rows unless that leaves fewer than four waves per SIMD
// (and the launch does not run beside other frames' launches), then 8.
void rcas_planar_geometry(int width, int height, int frames, bool overlapped, int* tiles_x, int* tiles_y, int* rows) {
  const int tx = (width + kRcasPlanarCols - 1) / kRcasPlanarCols;
  int r = 16;
  if (!overlapped && (long long)tx * ((height + r - 1) / r) * frames * kRcasPlanarWaves < 4LL * 4 * 256) r = 8;
  *rows = r;
  *tiles_x = tx;
  *tiles_y = (height + r - 1) / r;
}

// RING by the launch: the shallow ring when it is short of waves, fewer than 6 per SIMD in 16-row strips (rcas_launch's rule).  8-bit
// planes keep four rows in flight whatever the launch: packed, the deeper ring costs 4 registers (76 against 72, where fp16 pays 16),
// and a single 4K frame, the launch the rule calls short, measured 27.9 us with it against 31.0.
template <int FMT, bool EXACT, bool OPTS, bool WIDE>
static void rcas_planar_launch_one(const RcasArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasPlanarThreads);
  if constexpr (FMT != FSR1_FORMAT_RGB8_UNORM_PLANAR) {
    if ((long long)a.tiles_x * ((a.in.height + 15) / 16) * a.frames * kRcasPlanarWaves < 6LL * 4 * 256) {
      hipLaunchKernelGGL((rcas_planar_kernel<FMT, EXACT, OPTS, WIDE, 2>), grid, block, 0, stream, a);
      return;
    }
  }
  hipLaunchKernelGGL((rcas_planar_kernel<FMT, EXACT, OPTS, WIDE, 4>), grid, block, 0, stream, a);
}

// wide: the four-element accesses (the host has checked both images' base, pitch, plane and frame stride against them).
hipError_t rcas_planar_launch(const RcasArgs& a, int fmt, bool exact, bool wide, hipStream_t stream) {
  const bool opts = (a.flags & (FSR1_FLAG_RCAS_DENOISE | FSR1_FLAG_HDR_SQUARE)) != 0;
#define FSR1_RCASP(F, E, O, V) rcas_planar_launch_one<F, E, O, V>(a, stream)
#define FSR1_RCASP_V(F, E, O) do { if (wide) FSR1_RCASP(F, E, O, true); else FSR1_RCASP(F, E, O, false); } while (0)
#define FSR1_RCASP_O(F, E) do { if (opts) FSR1_RCASP_V(F, E, true); else FSR1_RCASP_V(F, E, false); } while (0)
#define FSR1_RCASP_E(F) do { if (exact) FSR1_RCASP_O(F, true); else FSR1_RCASP_O(F, false); } while (0)
  switch (fmt) {
    case FSR1_FORMAT_RGB16F_PLANAR: FSR1_RCASP_E(FSR1_FORMAT_RGB16F_PLANAR); break;
    case FSR1_FORMAT_RGB32F_PLANAR: FSR1_RCASP_E(FSR1_FORMAT_RGB32F_PLANAR); break;
    case FSR1_FORMAT_RGB8_UNORM_PLANAR: FSR1_RCASP_E(FSR1_FORMAT_RGB8_UNORM_PLANAR); break;
    default: return hipErrorInvalidValue;
  }
#undef FSR1_RCASP_E
#undef FSR1_RCASP_O
#undef FSR1_RCASP_V
#undef FSR1_RCASP
  return hipGetLastError();
}

}  // namespace fsr1
