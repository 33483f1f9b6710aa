// RCAS, packed binary16 arithmetic — FsrRcasHx2 (ffx-fsr/ffx_fsr1.h:888-984), whose per-element
// arithmetic is FsrRcasH (:782-866), for gfx950.
//
// Parity class "H": each lane sharpens TWO horizontally adjacent pixels in the two halves of packed
// binary16 registers (the reference pairs pixels 8 columns apart, :913; the pairing does not enter the
// arithmetic), one native binary16 operation per reference operation, contraction off — bit-identical
// to the reference's FsrRcasH evaluated on the CPU with round-to-nearest-even after every operation.
//
// Streaming structure of the fp32 kernel (fsr1_rcas.hip): no LDS, a wave owns a 128-column x 8-row strip,
// rows flow through registers (b = previous row, h = next row), the horizontal neighbours of a lane's
// pixel pair are its own other pixel and the adjacent lane's facing pixel (DPP wave shift); lanes 0 / 63
// also load the strip's apron column.  Loads outside the image are 0 (FSR_Pass.hlsl:61).
// That is the RGBA16F kernel (rcas_h_kernel); the 32 bpp UNORM formats have a strip shape of their own, four pixels per lane
// (rcas_h4_kernel, below), and RGBA16F in -> 32 bpp UNORM out, the TEPD target, a third (rcas_h4w_kernel: two 16-byte loads, one 16-byte
// store per lane-row).  Colour stages (class H, fsr1_device_color_half.hpp) are a compile-time switch of the first two and part of the third.
#include "fsr1_device.h"
#include "fsr1_device_half.hpp"

namespace fsr1 {

constexpr int kRcasHRows = 8;   // rows per strip, a multiple of the 4-row ring.  Measured at 4K, us (profiles/ab_r02/r2c9_ab.log): 8 rows 26.7, 16 rows 27.1, 32 rows 31.7; round 1's 24 rows x 4 waves, fully unrolled: 31.0
constexpr int kRcasHWaves = 2; // waves per workgroup, side by side: the F kernel's shape (fsr1_rcas_kernel.h)
constexpr int kRcasHThreads = 64 * kRcasHWaves;
constexpr int kRcasHCols = 128 * kRcasHWaves;  // columns per workgroup
constexpr int kShr1 = 0x138, kShl1 = 0x130;

namespace {

template <int CTRL>
__device__ __forceinline__ half2_t dpp2(half2_t keep, half2_t v) {
  return __builtin_bit_cast(half2_t, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, keep), __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

}  // namespace

// OPTS = false: plain pass, flags compiled out.
// COLOR (a compile-time switch; the stage-free kernels are the instantiations they were): the class-H colour stages of
// fsr1_device_color_half.hpp — FsrSrtmH where a row enters packed form (`load`: the ring holds post-SRTM values; a tap outside the image
// stays 0, FsrSrtmH(0) == 0), LFGA -> SRTM_INV -> TEPD on the sharpened pair (col, col + 1) in front of the store, after `c *= c`.
template <bool OPTS, bool COLOR>
__device__ __forceinline__ void rcas_h_strip(const RcasArgs& a) {
  const uint32_t flags = OPTS ? a.flags : 0u;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = tx * kRcasHCols + wave * 128, y0 = ty * kRcasHRows;
  if (x0 >= a.in.width) return;

  const int W = a.in.width, H = a.in.height;
  const int col = x0 + 2 * lane;
  const bool ok0 = col < W, ok1 = col + 1 < W;
  const int hcol = lane == 0 ? x0 - 1 : x0 + 128;
  const bool halo_ok = (lane == 0 || lane == 63) && hcol >= 0 && hcol < W;
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;

  // a row's address = wave-uniform 64-bit row base + a 32-bit lane offset (see rcas_strip in fsr1_rcas_kernel.h)
  const uint32_t off = (uint32_t)col * 8u, hoff = (uint32_t)max(hcol, 0) * 8u;
  auto zext = [](uint32_t o) { asm("" : "+v"(o)); return (size_t)o; };
  typedef TexelPair<FSR1_FORMAT_RGBA16F>::T pair_t;
  // one row of this lane's pixel pair as structure-of-arrays, plus the apron texel broadcast to both halves; the pair is
  // ONE 16-byte access (8-byte accesses run at 0.5-0.7 of the 16-byte rate on this chip)
  auto load = [&](int y, soa_t& own, soa_t& halo) {
    half4_t p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0}, ph = {0, 0, 0, 0};
    if (y >= 0 && y < H) {  // wave-uniform
      const char* const row = in_frame + (long long)y * a.in.pitch;
      if (ok1) {
        const pair_t pr = *reinterpret_cast<const pair_t*>(row + zext(off));
        p0 = half4_t{pr[0], pr[1], pr[2], pr[3]};
        p1 = half4_t{pr[4], pr[5], pr[6], pr[7]};
      } else if (ok0) {
        p0 = *reinterpret_cast<const half4_t*>(row + zext(off));
      }
      if (halo_ok) ph = *reinterpret_cast<const half4_t*>(row + zext(hoff));
    }
    own = soa_t{half2_t{p0.x, p1.x}, half2_t{p0.y, p1.y}, half2_t{p0.z, p1.z}, half2_t{p0.w, p1.w}};
    halo = soa_t{half2_t{ph.x, ph.x}, half2_t{ph.y, ph.y}, half2_t{ph.z, ph.z}, half2_t{ph.w, ph.w}};
    if constexpr (COLOR) {
      rgbh2_t c = {own.r, own.g, own.b}, ch = {halo.r, halo.g, halo.b};
      color_prologue_h2(a.color, c);
      color_prologue_h2(a.color, ch);
      own.r = c.r; own.g = c.g; own.b = c.b;
      halo.r = ch.r; halo.g = ch.g; halo.b = ch.b;
    }
  };

  constexpr int kAhead = 3, kRing = kAhead + 1;
  soa_t q[kRing], g[kRing];
  soa_t prev;
  {
    soa_t g_prev;
    load(y0 - 1, prev, g_prev);
#pragma unroll
    for (int k = 0; k < kAhead; ++k) load(y0 + k, q[k], g[k]);
  }
  // :857 sharpness = AH2_AU1(con.y).x — the packed half of con[1]
  const half_t sharp1 = __builtin_bit_cast(half_t, (u16)(a.con[1] & 0xffffu));
  const half2_t one = s2(1.0f);

  static_assert(kRcasHRows % kRing == 0, "strips are a multiple of the ring tall");
  // the row loop is unrolled by the ring (static ring indices) and rolled beyond that, so the body stays inside the
  // instruction cache (24 fully unrolled rows were 44 KB of code)
#pragma unroll 1
  for (int r0 = 0; r0 < kRcasHRows; r0 += kRing)
#pragma unroll
  for (int k = 0; k < kRing; ++k) {
    const int r = r0 + k;
    const int y = y0 + r;
    // (past the row below the strip nothing is needed: re-read that row — a cache hit — instead of fetching two more rows per
    //  strip from memory, which round 3's kernel did: 99.6 MB fetched per 4K frame against the F kernel's 83.1 MB)
    load(min(y + kAhead, y0 + kRcasHRows), q[(k + kAhead) % kRing], g[(k + kAhead) % kRing]);
    const soa_t& e = q[k % kRing];
    const soa_t& eh = g[k % kRing];
    const soa_t& h = q[(k + 1) % kRing];
    const soa_t& b = prev;
    // d = (left neighbour's right pixel, own left pixel) ; f = (own right pixel, right neighbour's left pixel)
    const half2_t nlR = dpp2<kShr1>(eh.r, e.r), nlG = dpp2<kShr1>(eh.g, e.g), nlB = dpp2<kShr1>(eh.b, e.b);
    const half2_t nrR = dpp2<kShl1>(eh.r, e.r), nrG = dpp2<kShl1>(eh.g, e.g), nrB = dpp2<kShl1>(eh.b, e.b);
    const half2_t dR = {nlR.y, e.r.x}, dG = {nlG.y, e.g.x}, dB = {nlB.y, e.b.x};
    const half2_t fR = {e.r.y, nrR.x}, fG = {e.g.y, nrG.x}, fB = {e.b.y, nrB.x};
    const half2_t bR = b.r, bG = b.g, bB = b.b, eR = e.r, eG = e.g, eB = e.b, hR = h.r, hG = h.g, hB = h.b;

    rgbh2_t px = rcas_pixel_h2(bR, bG, bB, dR, dG, dB, eR, eG, eB, fR, fG, fB, hR, hG, hB, sharp1, flags);
    if constexpr (COLOR) {
      if (a.color.stages & kColorEpilogue) color_epilogue_h2(a.color, (uint32_t)col, (uint32_t)col + 1u, (uint32_t)y, px);
    }
    const half2_t pR = px.r, pG = px.g, pB = px.b;
    const half2_t pA = (flags & FSR1_FLAG_RCAS_PASSTHROUGH_ALPHA) ? e.a : one;       // :905-907 / FSR_Pass.hlsl:94
    if (y < H) {
      char* const row = out_frame + (long long)y * a.out.pitch + zext(off);
      // FsrRcasDepackHx2 :880-886
      const half4_t t0 = {pR.x, pG.x, pB.x, pA.x}, t1 = {pR.y, pG.y, pB.y, pA.y};
      if (ok1) store_out<8>(row, TexelPair<FSR1_FORMAT_RGBA16F>::make(t0, t1), stream);
      else if (ok0) store_out<8>(row, t0, stream);
    }
    prev = e;
  }
}

template <bool OPTS>
__global__ void __launch_bounds__(kRcasHThreads) rcas_h_kernel(const RcasArgs a) {
  rcas_h_strip<OPTS, false>(a);
}
template <bool OPTS>
__global__ void __launch_bounds__(kRcasHThreads) rcas_h_color_kernel(const RcasArgs a) {
  rcas_h_strip<OPTS, true>(a);
}

// ---- 32 bpp UNORM storage (FSR1_FORMAT_RGBA8_UNORM, FSR1_FORMAT_R10G10B10A2_UNORM): FOUR adjacent pixels per lane ----
// 16-byte accesses are what this chip moves at full rate (above): at 4 bytes per pixel a lane therefore owns four pixels — one 16-byte load and one 16-byte store per lane-row — and a wave covers 256 columns.  A lane makes two
// rcas_pixel_h2 evaluations per row, on the pairs (p0, p1) and (p2, p3).  Their horizontal taps
//     d(p0,p1) = (left lane's p3, p0)     f(p0,p1) = (p1, p2) = d(p2,p3)     f(p2,p3) = (p3, right lane's p0)
// come from the lane's own registers except for two values, which cross by DPP wave shifts (three channels each: six v_mov_dpp per
// four pixels, where the two-pixel kernel spends six per two); lanes 0 / 63 load the strip's apron texel.
// Rows wait in the ring (kAhead rows in flight) as the codes they were loaded as — four registers and the apron's one — and are
// narrowed to binary16 pairs once, when they become the row below the centre; the centre and the row above are carried in registers.
// Alpha travels as the centre's code bits and only when FSR1_FLAG_RCAS_PASSTHROUGH_ALPHA asks for it (store(load(code)) == code for
// every code, fsr1_device_half.hpp), otherwise it is the constant maximum code: no alpha channel is ever converted.
// Strip shape: 8 rows, the RGBA16F kernel's measured optimum — the row above and the row below are read again by the neighbouring
// strips (+25 % of loads, cache hits for the most part), 16 rows and more lose more to the shorter grid than the apron saves, and a
// 4K image is 15 x 270 = 4050 waves, each with three 1 KB row loads in flight (12 MB outstanding: beyond the latency x bandwidth product
// of the memory system).  Two waves per workgroup, side by side, as in the other RCAS kernels; a wave whose 256 columns start beyond the
// image leaves at once.  Measured at 4K (profiles/unorm_h_1080p_to_4k.json, us): RGBA8 31.6 against the RGBA16F kernel's 32.3 in the
// same run — half the bytes, 2 % less time: with 16-byte accesses the pass is bound by the packed arithmetic (2.1 TB/s), not by memory.
// Other strip heights and a two-pixel / 8-byte form are unmeasured.
constexpr int kRcasH4Rows = 8;
constexpr int kRcasH4Waves = 2;
constexpr int kRcasH4Threads = 64 * kRcasH4Waves;
constexpr int kRcasH4WaveCols = 4 * 64;
constexpr int kRcasH4Cols = kRcasH4WaveCols * kRcasH4Waves;

// COLOR: as in rcas_h_strip — FsrSrtmH in `narrow` and on the apron texel, the epilogue on the pairs (col, col + 1) and (col + 2, col + 3).
template <int FMT, bool OPTS, bool COLOR>
__device__ __forceinline__ void rcas_h4_strip(const RcasArgs& a) {
  typedef TexelH<FMT> tex;
  typedef uint32_t quad_t __attribute__((ext_vector_type(4), aligned(4)));  // four texels: rows are only texel-aligned
  const uint32_t flags = OPTS ? a.flags : 0u;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = tx * kRcasH4Cols + wave * kRcasH4WaveCols, y0 = ty * kRcasH4Rows;
  if (x0 >= a.in.width) return;

  const int W = a.in.width, H = a.in.height;
  const int col = x0 + 4 * lane;
  const int nok = min(max(W - col, 0), 4);  // this lane's pixels inside the image: 4 but at a ragged right edge
  const int hcol = lane == 0 ? x0 - 1 : x0 + kRcasH4WaveCols;
  const bool halo_ok = (lane == 0 || lane == 63) && hcol >= 0 && hcol < W;
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;

  // a row's address = wave-uniform 64-bit row base + a 32-bit lane offset (see rcas_strip in fsr1_rcas_kernel.h)
  const uint32_t off = (uint32_t)col * 4u, hoff = (uint32_t)max(hcol, 0) * 4u;
  auto zext = [](uint32_t o) { asm("" : "+v"(o)); return (size_t)o; };
  struct raw_t { quad_t own; uint32_t halo; };
  // one row of this lane's four texels and the apron texel, as stored; code 0 (= 0.0 in every channel) outside the image (FSR_Pass.hlsl:61)
  auto load = [&](int y, raw_t& r) {
    quad_t p = {0u, 0u, 0u, 0u};
    uint32_t ph = 0u;
    if (y >= 0 && y < H) {  // wave-uniform
      const char* const row = in_frame + (long long)y * a.in.pitch;
      if (nok == 4) {
        p = *reinterpret_cast<const quad_t*>(row + zext(off));
      } else if (nok > 0) {
        const uint32_t* const px = reinterpret_cast<const uint32_t*>(row + zext(off));
        p.x = px[0];
        if (nok > 1) p.y = px[1];
        if (nok > 2) p.z = px[2];
      }
      if (halo_ok) ph = *reinterpret_cast<const uint32_t*>(row + zext(hoff));
    }
    r.own = p;
    r.halo = ph;
  };
  struct row_t { rgbh2_t lo, hi; };  // (p0, p1) and (p2, p3)
  auto narrow = [&](const quad_t& p) {
    row_t r = {tex::load_rgb2(p.x, p.y), tex::load_rgb2(p.z, p.w)};
    if constexpr (COLOR) {
      color_prologue_h2(a.color, r.lo);
      color_prologue_h2(a.color, r.hi);
    }
    return r;
  };

  constexpr int kAhead = 3, kRing = kAhead + 1;
  raw_t q[kRing];
  row_t b, e;
  {
    raw_t above;
    load(y0 - 1, above);
#pragma unroll
    for (int k = 0; k < kAhead; ++k) load(y0 + k, q[k]);
    b = narrow(above.own);
    e = narrow(q[0].own);
  }
  // :857 sharpness = AH2_AU1(con.y).x — the packed half of con[1]
  const half_t sharp1 = __builtin_bit_cast(half_t, (u16)(a.con[1] & 0xffffu));

  static_assert(kRcasH4Rows % kRing == 0, "strips are a multiple of the ring tall");
  // unrolled by the ring (static ring indices), rolled beyond that: see rcas_h_kernel
#pragma unroll 1
  for (int r0 = 0; r0 < kRcasH4Rows; r0 += kRing)
#pragma unroll
  for (int k = 0; k < kRing; ++k) {
    const int y = y0 + r0 + k;
    // (past the row below the strip nothing is needed: that row is read again — a cache hit — instead of two more rows per strip)
    load(min(y + kAhead, y0 + kRcasH4Rows), q[(k + kAhead) % kRing]);
    const row_t h = narrow(q[(k + 1) % kRing].own);
    const quad_t centre = q[k % kRing].own;
    rgbh2_t eh = tex::load_rgb2(q[k % kRing].halo, q[k % kRing].halo);  // the apron texel in both halves (lanes 0 / 63)
    if constexpr (COLOR) color_prologue_h2(a.color, eh);
    // the two values from the neighbouring lanes: .y of nl = the left lane's p3, .x of nr = the right lane's p0
    const half2_t nlR = dpp2<kShr1>(eh.r, e.hi.r), nlG = dpp2<kShr1>(eh.g, e.hi.g), nlB = dpp2<kShr1>(eh.b, e.hi.b);
    const half2_t nrR = dpp2<kShl1>(eh.r, e.lo.r), nrG = dpp2<kShl1>(eh.g, e.lo.g), nrB = dpp2<kShl1>(eh.b, e.lo.b);
    const half2_t dR = {nlR.y, e.lo.r.x}, dG = {nlG.y, e.lo.g.x}, dB = {nlB.y, e.lo.b.x};   // left of (p0, p1)
    const half2_t mR = {e.lo.r.y, e.hi.r.x}, mG = {e.lo.g.y, e.hi.g.x}, mB = {e.lo.b.y, e.hi.b.x};  // (p1, p2): right of (p0, p1), left of (p2, p3)
    const half2_t fR = {e.hi.r.y, nrR.x}, fG = {e.hi.g.y, nrG.x}, fB = {e.hi.b.y, nrB.x};   // right of (p2, p3)
    rgbh2_t lo = rcas_pixel_h2(b.lo.r, b.lo.g, b.lo.b, dR, dG, dB, e.lo.r, e.lo.g, e.lo.b, mR, mG, mB, h.lo.r, h.lo.g, h.lo.b, sharp1, flags);
    rgbh2_t hi = rcas_pixel_h2(b.hi.r, b.hi.g, b.hi.b, mR, mG, mB, e.hi.r, e.hi.g, e.hi.b, fR, fG, fB, h.hi.r, h.hi.g, h.hi.b, sharp1, flags);
    if constexpr (COLOR) {
      if (a.color.stages & kColorEpilogue) {
        color_epilogue_h2(a.color, (uint32_t)col, (uint32_t)col + 1u, (uint32_t)y, lo);
        color_epilogue_h2(a.color, (uint32_t)col + 2u, (uint32_t)col + 3u, (uint32_t)y, hi);
      }
    }
    if (y < H && nok > 0) {  // (y < H: wave-uniform)
      // alpha: the centre's own code, or the maximum code (:905-907 / FSR_Pass.hlsl:94)
      const bool pass_alpha = (flags & FSR1_FLAG_RCAS_PASSTHROUGH_ALPHA) != 0;
      const quad_t alpha = pass_alpha ? (quad_t)(centre & tex::kAlphaMask) : quad_t{tex::kAlphaMask, tex::kAlphaMask, tex::kAlphaMask, tex::kAlphaMask};
      const quad_t o = quad_t{tex::store_rgb(lo.r.x, lo.g.x, lo.b.x), tex::store_rgb(lo.r.y, lo.g.y, lo.b.y),
                              tex::store_rgb(hi.r.x, hi.g.x, hi.b.x), tex::store_rgb(hi.r.y, hi.g.y, hi.b.y)} | alpha;
      char* const row = out_frame + (long long)y * a.out.pitch + zext(off);
      if (nok == 4) {
        store_out<4>(row, o, stream);
      } else {  // ragged right edge: 1 - 3 pixels, a texel at a time
        store_out<4>(row, (uint32_t)o.x, stream);
        if (nok > 1) store_out<4>(row + 4, (uint32_t)o.y, stream);
        if (nok > 2) store_out<4>(row + 8, (uint32_t)o.z, stream);
      }
    }
    b = e;
    e = h;
  }
}

template <int FMT, bool OPTS>
__global__ void __launch_bounds__(kRcasH4Threads) rcas_h4_kernel(const RcasArgs a) {
  rcas_h4_strip<FMT, OPTS, false>(a);
}
template <int FMT, bool OPTS>
__global__ void __launch_bounds__(kRcasH4Threads) rcas_h4_color_kernel(const RcasArgs a) {
  rcas_h4_strip<FMT, OPTS, true>(a);
}

// ---- RGBA16F in -> 32 bpp UNORM out, with colour stages: the TEPD target, the final pass of the SDR chain (HDR render target -> EASU ->
// RCAS -> grain -> TEPD -> 8 / 10-bit swap chain) ----
// Neither shape above fits: two pixels per lane give 16-byte loads but 8-byte stores (0.5-0.7 of the 16-byte rate), and the four-pixel
// kernel loads 4 bytes per pixel.  Here a lane owns four adjacent pixels as in rcas_h4_strip — the same taps from the same places, two
// values per channel crossing by DPP wave shift, lanes 0 / 63 loading the apron texel, a wave 256 columns wide, 8-row strips, two waves
// side by side — and per row issues TWO 16-byte loads (its 32 contiguous bytes) and ONE 16-byte store.
// The ring holds the rows AS LOADED (eight registers and the apron's two), not as packed pairs (six): a row can only be repacked once
// its loads have landed, so a ring of packed rows would wait for every load where it is issued and keep nothing in flight; the registers
// a load targets are occupied from its issue in either form.  A row is transposed to (p0, p1) / (p2, p3) channel pairs — and tone-mapped,
// when FSR1_COLOR_SRTM asks for it — once, when it becomes the row below the centre; the centre and the row above are carried as pairs
// (12 registers), the centre's alpha is read from its ring slot only under FSR1_FLAG_RCAS_PASSTHROUGH_ALPHA.  40 ring registers against
// the four-pixel UNORM kernel's 20: the register counts are in DESIGN.md section 3.4 (no scratch).
// The epilogue (LFGA -> SRTM_INV -> TEPD, after `c *= c`) runs on the pairs (col, col + 1) and (col + 2, col + 3).
template <int FOUT, bool OPTS>
__global__ void __launch_bounds__(kRcasH4Threads) rcas_h4w_kernel(const RcasArgs a) {
  typedef TexelH<FOUT> tex;
  typedef uint32_t quad_t __attribute__((ext_vector_type(4), aligned(4)));   // four stored texels
  typedef uint32_t pair32_t __attribute__((ext_vector_type(4), aligned(8)));  // two RGBA16F texels: (R | G << 16, B | A << 16) each
  typedef uint32_t texel_t __attribute__((ext_vector_type(2), aligned(8)));  // one
  const uint32_t flags = OPTS ? a.flags : 0u;
  const bool stream = (a.flags & FSR1_FLAG_OUTPUT_STREAMING) != 0;
  const int tiles_per_frame = a.tiles_x * a.tiles_y;
  const int t = xcd_swizzle(blockIdx.x, tiles_per_frame * a.frames, a.xcd_shift);
  const int frame = t / tiles_per_frame;
  const int tf = t - frame * tiles_per_frame;
  const int ty = tf / a.tiles_x, tx = tf - ty * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = tx * kRcasH4Cols + wave * kRcasH4WaveCols, y0 = ty * kRcasH4Rows;
  if (x0 >= a.in.width) return;

  const int W = a.in.width, H = a.in.height;
  const int col = x0 + 4 * lane;
  const int nok = min(max(W - col, 0), 4);  // this lane's pixels inside the image: 4 but at a ragged right edge
  const int hcol = lane == 0 ? x0 - 1 : x0 + kRcasH4WaveCols;
  const bool halo_ok = (lane == 0 || lane == 63) && hcol >= 0 && hcol < W;
  const char* const in_frame = a.in.base + (long long)frame * a.in.frame_stride;
  char* const out_frame = a.out.base + (long long)frame * a.out.frame_stride;

  // a row's address = wave-uniform 64-bit row base + a 32-bit lane offset (see rcas_strip in fsr1_rcas_kernel.h)
  const uint32_t off = (uint32_t)col * 8u, hoff = (uint32_t)max(hcol, 0) * 8u, ooff = (uint32_t)col * 4u;
  auto zext = [](uint32_t o) { asm("" : "+v"(o)); return (size_t)o; };
  struct raw_t { pair32_t lo, hi; texel_t halo; };  // texels (p0, p1), (p2, p3) and the apron texel, as stored
  // one row of this lane's four texels and the apron texel; 0 (= 0.0 in every channel) outside the image (FSR_Pass.hlsl:61)
  auto load = [&](int y, raw_t& r) {
    pair32_t lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
    texel_t ph = {0u, 0u};
    if (y >= 0 && y < H) {  // wave-uniform
      const char* const row = in_frame + (long long)y * a.in.pitch;
      if (nok == 4) {
        const pair32_t* const px = reinterpret_cast<const pair32_t*>(row + zext(off));
        lo = px[0];
        hi = px[1];
      } else if (nok > 0) {  // ragged right edge: 1 - 3 pixels, a texel at a time
        const texel_t* const px = reinterpret_cast<const texel_t*>(row + zext(off));
        const texel_t t0 = px[0];
        lo.x = t0.x; lo.y = t0.y;
        if (nok > 1) { const texel_t t1 = px[1]; lo.z = t1.x; lo.w = t1.y; }
        if (nok > 2) { const texel_t t2 = px[2]; hi.x = t2.x; hi.y = t2.y; }
      }
      if (halo_ok) ph = *reinterpret_cast<const texel_t*>(row + zext(hoff));
    }
    r.lo = lo;
    r.hi = hi;
    r.halo = ph;
  };
  // two stored texels (rg0, ba0), (rg1, ba1) -> their channels as pairs, tone-mapped when the prologue asks for it
  auto pack = [&](uint32_t rg0, uint32_t ba0, uint32_t rg1, uint32_t ba1) {
    const half2_t a0 = as_h2(rg0), b0 = as_h2(ba0), a1 = as_h2(rg1), b1 = as_h2(ba1);
    rgbh2_t c = {half2_t{a0.x, a1.x}, half2_t{a0.y, a1.y}, half2_t{b0.x, b1.x}};
    color_prologue_h2(a.color, c);
    return c;
  };
  struct row_t { rgbh2_t lo, hi; };  // (p0, p1) and (p2, p3)
  auto narrow = [&](const raw_t& r) { return row_t{pack(r.lo.x, r.lo.y, r.lo.z, r.lo.w), pack(r.hi.x, r.hi.y, r.hi.z, r.hi.w)}; };

  constexpr int kAhead = 3, kRing = kAhead + 1;
  raw_t q[kRing];
  row_t b, e;
  {
    raw_t above;
    load(y0 - 1, above);
#pragma unroll
    for (int k = 0; k < kAhead; ++k) load(y0 + k, q[k]);
    b = narrow(above);
    e = narrow(q[0]);
  }
  // :857 sharpness = AH2_AU1(con.y).x — the packed half of con[1]
  const half_t sharp1 = __builtin_bit_cast(half_t, (u16)(a.con[1] & 0xffffu));
  const bool epilogue = (a.color.stages & kColorEpilogue) != 0;

  static_assert(kRcasH4Rows % kRing == 0, "strips are a multiple of the ring tall");
  // unrolled by the ring (static ring indices), rolled beyond that: see rcas_h_kernel
#pragma unroll 1
  for (int r0 = 0; r0 < kRcasH4Rows; r0 += kRing)
#pragma unroll
  for (int k = 0; k < kRing; ++k) {
    const int y = y0 + r0 + k;
    // (past the row below the strip nothing is needed: that row is read again — a cache hit — instead of two more rows per strip)
    load(min(y + kAhead, y0 + kRcasH4Rows), q[(k + kAhead) % kRing]);
    const row_t h = narrow(q[(k + 1) % kRing]);
    const raw_t& centre = q[k % kRing];
    const rgbh2_t eh = pack(centre.halo.x, centre.halo.y, centre.halo.x, centre.halo.y);  // the apron texel in both halves (lanes 0 / 63)
    // the two values from the neighbouring lanes: .y of nl = the left lane's p3, .x of nr = the right lane's p0
    const half2_t nlR = dpp2<kShr1>(eh.r, e.hi.r), nlG = dpp2<kShr1>(eh.g, e.hi.g), nlB = dpp2<kShr1>(eh.b, e.hi.b);
    const half2_t nrR = dpp2<kShl1>(eh.r, e.lo.r), nrG = dpp2<kShl1>(eh.g, e.lo.g), nrB = dpp2<kShl1>(eh.b, e.lo.b);
    const half2_t dR = {nlR.y, e.lo.r.x}, dG = {nlG.y, e.lo.g.x}, dB = {nlB.y, e.lo.b.x};   // left of (p0, p1)
    const half2_t mR = {e.lo.r.y, e.hi.r.x}, mG = {e.lo.g.y, e.hi.g.x}, mB = {e.lo.b.y, e.hi.b.x};  // (p1, p2): right of (p0, p1), left of (p2, p3)
    const half2_t fR = {e.hi.r.y, nrR.x}, fG = {e.hi.g.y, nrG.x}, fB = {e.hi.b.y, nrB.x};   // right of (p2, p3)
    rgbh2_t lo = rcas_pixel_h2(b.lo.r, b.lo.g, b.lo.b, dR, dG, dB, e.lo.r, e.lo.g, e.lo.b, mR, mG, mB, h.lo.r, h.lo.g, h.lo.b, sharp1, flags);
    rgbh2_t hi = rcas_pixel_h2(b.hi.r, b.hi.g, b.hi.b, mR, mG, mB, e.hi.r, e.hi.g, e.hi.b, fR, fG, fB, h.hi.r, h.hi.g, h.hi.b, sharp1, flags);
    if (epilogue) {  // (the noise tile wraps, so the positions of a ragged lane's missing pixels are fetched harmlessly)
      color_epilogue_h2(a.color, (uint32_t)col, (uint32_t)col + 1u, (uint32_t)y, lo);
      color_epilogue_h2(a.color, (uint32_t)col + 2u, (uint32_t)col + 3u, (uint32_t)y, hi);
    }
    if (y < H && nok > 0) {  // (y < H: wave-uniform)
      // alpha: the centre's binary16 alpha through the store rule, or the maximum code (:905-907 / FSR_Pass.hlsl:94)
      quad_t alpha = {tex::kAlphaMask, tex::kAlphaMask, tex::kAlphaMask, tex::kAlphaMask};
      if (flags & FSR1_FLAG_RCAS_PASSTHROUGH_ALPHA) {
        auto code = [](uint32_t ba) { return (uint32_t)Pixel<FOUT>::store(0.0f, 0.0f, 0.0f, (float)as_h2(ba).y); };
        alpha = quad_t{code(centre.lo.y), code(centre.lo.w), code(centre.hi.y), code(centre.hi.w)};
      }
      const quad_t o = quad_t{tex::store_rgb(lo.r.x, lo.g.x, lo.b.x), tex::store_rgb(lo.r.y, lo.g.y, lo.b.y),
                              tex::store_rgb(hi.r.x, hi.g.x, hi.b.x), tex::store_rgb(hi.r.y, hi.g.y, hi.b.y)} | alpha;
      char* const row = out_frame + (long long)y * a.out.pitch + zext(ooff);
      if (nok == 4) {
        store_out<4>(row, o, stream);
      } else {  // ragged right edge: 1 - 3 pixels, a texel at a time
        store_out<4>(row, (uint32_t)o.x, stream);
        if (nok > 1) store_out<4>(row + 4, (uint32_t)o.y, stream);
        if (nok > 2) store_out<4>(row + 8, (uint32_t)o.z, stream);
      }
    }
    b = e;
    e = h;
  }
}

// RGBA16F in and out takes the two-pixel strips, every other pair (a 32 bpp UNORM format on either side) the four-pixel strips
void rcas_h_geometry(int fmt, int fout, int width, int height, int* tiles_x, int* tiles_y) {
  const bool two = fmt == FSR1_FORMAT_RGBA16F && fout == FSR1_FORMAT_RGBA16F;
  const int cols = two ? kRcasHCols : kRcasH4Cols, rows = two ? kRcasHRows : kRcasH4Rows;
  *tiles_x = (width + cols - 1) / cols;
  *tiles_y = (height + rows - 1) / rows;
}

namespace {
template <int FMT>
hipError_t rcas_h4_launch(const RcasArgs& a, bool opts, bool color, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasH4Threads);
  if (color) {
    if (opts) hipLaunchKernelGGL((rcas_h4_color_kernel<FMT, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((rcas_h4_color_kernel<FMT, false>), grid, block, 0, stream, a);
  } else {
    if (opts) hipLaunchKernelGGL((rcas_h4_kernel<FMT, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((rcas_h4_kernel<FMT, false>), grid, block, 0, stream, a);
  }
  return hipGetLastError();
}
template <int FOUT>
hipError_t rcas_h4w_launch(const RcasArgs& a, bool opts, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasH4Threads);
  if (opts) hipLaunchKernelGGL((rcas_h4w_kernel<FOUT, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((rcas_h4w_kernel<FOUT, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}
}  // namespace

// The kernel follows from (input format, output format, colour stages); a launch without stages (fout == fmt) takes the stage-free kernels.
hipError_t rcas_h_launch(const RcasArgs& a0, int fmt, int fout, hipStream_t stream) {
  RcasArgs a = a0;
  rcas_h_geometry(fmt, fout, a.in.width, a.in.height, &a.tiles_x, &a.tiles_y);  // its own strip shapes (two / four pixels per lane)
  const bool opts = (a.flags & (FSR1_FLAG_RCAS_DENOISE | FSR1_FLAG_RCAS_PASSTHROUGH_ALPHA | FSR1_FLAG_HDR_SQUARE)) != 0;
  const bool color = a.color.stages != 0;
  if (fout != fmt) {  // RGBA16F -> a TEPD target
    if (!color || fmt != FSR1_FORMAT_RGBA16F) return hipErrorInvalidValue;
    if (fout == FSR1_FORMAT_RGBA8_UNORM) return rcas_h4w_launch<FSR1_FORMAT_RGBA8_UNORM>(a, opts, stream);
    if (fout == FSR1_FORMAT_R10G10B10A2_UNORM) return rcas_h4w_launch<FSR1_FORMAT_R10G10B10A2_UNORM>(a, opts, stream);
    return hipErrorInvalidValue;
  }
  if (fmt == FSR1_FORMAT_RGBA8_UNORM) return rcas_h4_launch<FSR1_FORMAT_RGBA8_UNORM>(a, opts, color, stream);
  if (fmt == FSR1_FORMAT_R10G10B10A2_UNORM) return rcas_h4_launch<FSR1_FORMAT_R10G10B10A2_UNORM>(a, opts, color, stream);
  if (fmt != FSR1_FORMAT_RGBA16F) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasHThreads);
  if (color) {
    if (opts) hipLaunchKernelGGL(rcas_h_color_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(rcas_h_color_kernel<false>, grid, block, 0, stream, a);
  } else {
    if (opts) hipLaunchKernelGGL(rcas_h_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(rcas_h_kernel<false>, grid, block, 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace fsr1
