// The RCAS strip of single-channel images, shared by the kernels that run it: rcas_mono_kernel (fsr1_rcas_mono.hip) and the luma-domain
// transcode's second launch (fsr1_rcas_luma.hip), whose first workgroups are these strips on the Y plane.  No LDS, no barrier.
//   * a wave owns a strip of 64 G columns and walks it row by row — downwards in even strip rows, upwards in odd ones, so that
//     vertically adjacent strips meet at the rows they share; a lane owns G adjacent columns (MonoGroup): per row ONE load and one
//     store of G elements.  G and the strip height are the launch shape, measured (kRcasMonoCols, rcas_mono_geometry): a 4K frame is
//     8.3 M pixels and 33 MB moved, and what paces the pass is the number of independent row streams in flight, not bytes (DESIGN.md
//     3.2, 3.5c);
//   * of the horizontal taps of a lane's G pixels all but two are its own registers; the two are the facing pixels of the adjacent
//     lanes, fetched in fp32 by DPP wave shifts: two moves per G pixels;
//   * lanes 0 and 63 load the apron column, one element, which the DPP move leaves in place for exactly those lanes;
//   * rows live in a register ring: prev / cur / next as fp32, raw rows in flight ahead of the arithmetic, packed as in memory
//     (G * element size / 4 registers a row; uint8: four columns a register, decoded once, as the row becomes `next`);
//   * the per-pixel function is rcas_mono_pixel<EXACT>: channel R of rcas_pixel<EXACT> on the replicated taps, bit for bit;
//   * taps outside the image are 0; strips wholly inside the image run a branch-free body, the image's first / last wave-column the
//     same body with its apron texel replaced, everything else a fully predicated one;
//   * WIDE = false — base, pitch or frame stride not a multiple of the group's access — moves every element by itself: no access is
//     ever wider than its alignment, and with WIDE none is narrower than 4 bytes.
#pragma once
#include "fsr1_device.h"
#include "fsr1_device_mono.hpp"

namespace fsr1 {

constexpr int kRcasMonoWaves = 2;  // waves per workgroup, side by side
constexpr int kRcasMonoThreads = 64 * kRcasMonoWaves;
constexpr int kRcasMonoRing = 4;   // raw rows in flight per lane; divides every strip height (8, 16)

template <int FMT, bool EXACT, bool OPTS, bool WIDE, bool INTERIOR, int RING, int G, bool XEDGE = false, bool UP = false>
__device__ __forceinline__ void rcas_mono_strip(const RcasArgs& a, int frame, int x0, int y0, int lane) {
  typedef typename Mono<FMT>::U elem_t;
  typedef MonoGroup<FMT, G> group_t;
  constexpr int kWaveCols = 64 * G;
  const uint32_t flags = OPTS ? a.flags : 0u;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  const int W = a.in.width, H = a.in.height;
  const int col = x0 + G * lane;
  const bool all_in = INTERIOR || col + G <= W;  // the lane's whole group lies inside the image
  const bool edge = lane == 0 || lane == 63;
  // apron column of lanes 0 / 63; the other lanes point at their own column, so that the interior body loads unconditionally
  const int hcol = lane == 0 ? x0 - 1 : (lane == 63 ? x0 + kWaveCols : col);
  const bool halo_ok = edge && ((INTERIOR && !XEDGE) || (hcol >= 0 && hcol < W));
  const bool halo_out = XEDGE && edge && !halo_ok;  // (an outside apron texel is never addressed: its lane re-reads column 0 / W - 1)
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;
  const uint32_t off = (uint32_t)col * (uint32_t)sizeof(elem_t), hoff = (uint32_t)min(max(hcol, 0), W - 1) * (uint32_t)sizeof(elem_t);
  auto zext = [](uint32_t o) { asm("" : "+v"(o)); return (size_t)o; };  // (keeps the lane offset next to its use: fsr1_rcas_kernel.h)

  const int rows = a.rows;
  static_assert(!UP || INTERIOR, "only strips that store every row walk up");
  auto row_y = [&](int k) { return UP ? y0 + rows - 1 - k : y0 + k; };  // k-th row of the walk, k = -1 .. rows
  struct row_t { group_t g; elem_t halo; };
  // element I of a group, by itself: the narrow form and the lanes the image's right edge cuts
  auto load_elems = [&](const char* p, group_t& g, auto in) {
    const elem_t* const e = reinterpret_cast<const elem_t*>(p);
#pragma unroll
    for (int i = 0; i < G; ++i)
      if (in(i)) g.put(i, e[i]);
  };
  auto store_elems = [&](char* p, const group_t& g, auto in) {
#pragma unroll
    for (int i = 0; i < G; ++i)
      if (in(i)) store_out<sizeof(elem_t)>(p + i * sizeof(elem_t), g.elem(i), stream);
  };
  auto load = [&](int y, row_t& r) {
    const bool row_in = INTERIOR || (y >= 0 && y < H);  // wave-uniform
    const char* const src = in_frame + (long long)y * a.in.pitch;  // scalar
    if (INTERIOR) {
      if constexpr (WIDE) {
        r.g.load_wide(src + zext(off));
      } else {
        r.g.clear();
        load_elems(src + zext(off), r.g, [](int) { return true; });
      }
      r.halo = *reinterpret_cast<const elem_t*>(src + zext(hoff));
      if constexpr (XEDGE) {
        if (halo_out) r.halo = (elem_t)0;
      }
    } else {
      r.g.clear();
      r.halo = (elem_t)0;
      if (row_in) {
        if (WIDE && all_in) r.g.load_wide(src + zext(off));
        else load_elems(src + zext(off), r.g, [&](int i) { return col + i < W; });
        if (halo_ok) r.halo = *reinterpret_cast<const elem_t*>(src + zext(hoff));
      }
    }
  };
  struct px_t { float v[G]; };
  auto decode = [](const row_t& r) {
    px_t p;
#pragma unroll
    for (int i = 0; i < G; ++i) p.v[i] = r.g.get(i);
    return p;
  };
  // ring of raw rows in registers, loads kAhead rows ahead of the arithmetic; the row loop is unrolled by the ring (static indices)
  constexpr int kRing = RING, kAhead = kRing - 1;
  row_t q[kRing];
  px_t prev, cur;
  {
    row_t q_prev;
    load(row_y(-1), q_prev);
#pragma unroll
    for (int k = 0; k < kAhead; ++k) load(row_y(k), q[k]);
    prev = decode(q_prev);
    cur = decode(q[0]);
  }
  const float sharp = as_f32(a.con[0]);

#pragma unroll 1
  for (int r0 = 0; r0 < rows; r0 += kRing) {
#pragma unroll
    for (int k = 0; k < kRing; ++k) {
      const int y = row_y(r0 + k);
      load(row_y(min(r0 + k + kAhead, rows)), q[(k + kAhead) % kRing]);  // past the end: re-reads the last row (harmless, branch-free)
      const px_t next = decode(q[(k + 1) % kRing]);
      const float hal = Mono<FMT>::load(q[k].halo);
      // pixel 0's left tap = the left lane's last pixel, the last pixel's right tap = the right lane's pixel 0; lanes 0 / 63 keep their apron texel
      const float left = dpp_f32<kDppWaveShr1>(hal, cur.v[G - 1]), right = dpp_f32<kDppWaveShl1>(hal, cur.v[0]);
      const px_t& above = UP ? next : prev;  // b is the tap above, h the one below (ffx_fsr1.h:697-707), whichever way the strip walks
      const px_t& below = UP ? prev : next;
      float out[G];
#pragma unroll
      for (int i = 0; i < G; ++i)
        out[i] = rcas_mono_pixel<EXACT>(above.v[i], i ? cur.v[i - 1] : left, cur.v[i], i + 1 < G ? cur.v[i + 1] : right, below.v[i], sharp, flags);
      if (INTERIOR || y < H) {
        char* const dst = out_frame + (long long)y * a.out.pitch + zext(off);
        const group_t g = group_t::pack(out);
        if (WIDE && all_in) g.store_wide(dst, stream);
        else store_elems(dst, g, [&](int i) { return INTERIOR || col + i < W; });
      }
      prev = cur;
      cur = next;
    }
  }
}

// Tile t of the tiles_x * tiles_y * frames strips of a launch: which wave-column and strip row it is, and the body that serves it.
template <int FMT, bool EXACT, bool OPTS, bool WIDE, int RING, int G>
__device__ __forceinline__ void rcas_mono_tile(const RcasArgs& a, int t) {
  constexpr int kWaveCols = 64 * G;
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (tx * kRcasMonoWaves + wave) * kWaveCols, y0 = ty * a.rows;
  if (x0 >= a.in.width) return;  // whole wave outside (no barriers in this kernel)
  const bool interior_y = y0 >= 1 && y0 + a.rows + 1 <= a.in.height;  // every row the strip reads and stores is inside
  const bool inside_x = x0 + kWaveCols <= a.in.width;
  const bool interior = interior_y && x0 >= 1 && x0 + kWaveCols + 1 <= a.in.width;
  const bool up = (ty & 1) != 0;
  if (interior && up) rcas_mono_strip<FMT, EXACT, OPTS, WIDE, true, RING, G, false, true>(a, frame, x0, y0, lane);
  else if (interior) rcas_mono_strip<FMT, EXACT, OPTS, WIDE, true, RING, G>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x && up) rcas_mono_strip<FMT, EXACT, OPTS, WIDE, true, RING, G, true, true>(a, frame, x0, y0, lane);
  else if (interior_y && inside_x) rcas_mono_strip<FMT, EXACT, OPTS, WIDE, true, RING, G, true>(a, frame, x0, y0, lane);
  else rcas_mono_strip<FMT, EXACT, OPTS, WIDE, false, RING, G>(a, frame, x0, y0, lane);
}

// Columns a lane owns: the 8-byte access (binary16: 4, binary32: 2) and, for uint8, the dword (4) — measured at 3840 x 2160 against the
// group of twice the width (the 16-byte access; uint8: 8 bytes) at strips of 16 / 8 / 4 rows, us per call, binary16 | uint8
// (profiles/mono_rcas_shapes_4k.json): this group 14.6 / 12.2 / 12.8 | 16.1 / 12.5 / 12.6, the wider one 21.1 / 15.6 / 12.4 | 22.5 / 16.1 / 12.9.
// The pass is paced by its row streams (waves), not by the width of its accesses: the wider group is not built.
template <int FMT> constexpr int kRcasMonoCols = FMT == FSR1_FORMAT_R32F ? 2 : 4;

}  // namespace fsr1
