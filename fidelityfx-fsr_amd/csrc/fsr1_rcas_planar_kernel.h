// The strip walk of RCAS on planar RGB input, shared by the kernels that differ in what they do with a finished row:
// fsr1_rcas_planar.hip stores it as three planes of the input's type, fsr1_rcas_nv12.hip converts it to an NV12 surface.
//   * a wave owns a 256-column strip and walks it row by row — downwards in even strip rows, upwards in odd ones, so that vertically
//     adjacent strips meet at the rows they share (fsr1_rcas_kernel.h, UP); a lane owns FOUR adjacent columns: per row and plane one
//     8-byte (fp16) or 16-byte (fp32) load; 8-bit planes: one DWORD, the raw rows stay in flight as packed dwords (three registers a
//     row) and a row is decoded once, as it becomes `next`;
//   * of the horizontal taps of a lane's four pixels, six are its own registers and two are the facing pixels of the adjacent lanes,
//     fetched in fp32 by DPP wave shifts: six moves per four pixels (the interleaved kernel: six per two);
//   * lanes 0 and 63 load the apron column, one element per plane, which the DPP move leaves in place for exactly those lanes;
//   * rows live in a register ring: prev / cur / next as fp32, raw rows in flight ahead of the arithmetic (2 deep for a launch short
//     of waves, 4 for batches; 8-bit planes: always 4);
//   * the per-pixel function is rcas_pixel<EXACT> with the interleaved kernel's operand order (b above, h below whichever way the
//     strip walks): every value is the one that kernel stores for the same pixels with alpha 1;
//   * taps outside the image are 0; strips wholly inside the image run a branch-free body, the image's first / last wave-column the
//     same body with its apron texel replaced, everything else a fully predicated one.
// SINK: what becomes of a row.  SINK(args, frame) is built once per strip; for every row of the walk that lies in the image the strip
// calls sink.row<INTERIOR, UP>(k, y, col, off, ok, o0, o1, o2, o3): k = the row's index in the walk (static after unrolling; the ring is
// even and strips start on multiples of 8, so rows k, k + 1 with k even are the two rows of one 2 x 2 block row whichever way the
// strip walks), y = its image row, col = the lane's first column and off = its byte offset in an INPUT plane row, ok[i] = column i of the
// lane is inside the image, o0 .. o3 = the four binary32 results.
#pragma once
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

// (keeps the lane offset next to its use: fsr1_rcas_kernel.h)
__device__ __forceinline__ size_t rcas_planar_zext(uint32_t o) { asm("" : "+v"(o)); return (size_t)o; }

template <int FMT, bool EXACT, bool OPTS, bool WIDE, bool INTERIOR, int RING, class SINK, bool XEDGE = false, bool UP = false, class ARGS>
__device__ __forceinline__ void rcas_planar_strip(const ARGS& a, int frame, int x0, int y0, int lane) {
  typedef typename Plane<FMT>::E elem_t;
  typedef typename Plane<FMT>::V4 quad_t;
  const uint32_t flags = OPTS ? a.flags : 0u;
  const int W = a.in.width, H = a.in.height;
  const int col = x0 + 4 * lane;
  const bool ok[4] = {INTERIOR || col < W, INTERIOR || col + 1 < W, INTERIOR || col + 2 < W, INTERIOR || col + 3 < W};
  const bool edge = lane == 0 || lane == 63;
  // apron column of lanes 0 / 63; the other lanes point at their own column, so that the interior body loads unconditionally
  const int hcol = lane == 0 ? x0 - 1 : (lane == 63 ? x0 + kRcasPlanarWaveCols : col);
  const bool halo_ok = edge && ((INTERIOR && !XEDGE) || (hcol >= 0 && hcol < W));
  const bool halo_out = XEDGE && edge && !halo_ok;  // (an outside apron texel is never addressed: its lane re-reads column 0 / W - 1)
  const long long ips = plane_stride(a.in);
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  SINK sink(a, frame);
  const uint32_t off = (uint32_t)col * (uint32_t)sizeof(elem_t), hoff = (uint32_t)min(max(hcol, 0), W - 1) * (uint32_t)sizeof(elem_t);
  auto zext = [](uint32_t o) { return rcas_planar_zext(o); };

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
  static_assert(kRing % 2 == 0, "a sink pairs rows k, k + 1 of the walk");
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
      if (INTERIOR || y < H) sink.template row<INTERIOR, UP>(k, y, col, off, ok, o0, o1, o2, o3);
      prev = cur;
      cur = next;
    }
  }
}

// A workgroup's strip, by the XCD-aware order, and the body it takes.
template <int FMT, bool EXACT, bool OPTS, bool WIDE, int RING, class SINK, class ARGS>
__device__ __forceinline__ void rcas_planar_workgroup(const ARGS& a) {
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
  if (interior && up) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING, SINK, false, true>(a, frame, x0, y0, lane);
  else if (interior) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING, SINK>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x && up) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING, SINK, true, true>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x) rcas_planar_strip<FMT, EXACT, OPTS, WIDE, true, RING, SINK, true>(a, frame, x0, y0, lane);
  else rcas_planar_strip<FMT, EXACT, OPTS, WIDE, false, RING, SINK>(a, frame, x0, y0, lane);
}

// RING by the launch: the shallow ring when it is short of waves, fewer than 6 per SIMD in 16-row strips (rcas_launch's rule).  8-bit
// planes keep four rows in flight whatever the launch: packed, the deeper ring costs 4 registers (76 against 72, where fp16 pays 16),
// and a single 4K frame, the launch the rule calls short, measured 27.9 us with it against 31.0.
inline bool rcas_planar_shallow_ring(const RcasArgs& a, int fmt) {
  return fmt != FSR1_FORMAT_RGB8_UNORM_PLANAR && (long long)a.tiles_x * ((a.in.height + 15) / 16) * a.frames * kRcasPlanarWaves < 6LL * 4 * 256;
}

}  // namespace fsr1
