// Single-channel storage (FSR1_FORMAT_R16F / R32F / R8_UNORM) for the tiled forms: one plane of `height` rows, rows `pitch` bytes apart.
// The output for a luma image L is channel R of FsrEasuF / FsrRcasF on the image (L, L, L, 1) — and, in the default arithmetic, channel R
// of what the RGBA kernels store for it: every function below performs, on its one channel, the operations the three-channel function
// it is named after performs on channel R, in the same order.  What differs from the RGBA / planar kernels is everything around that:
//   * the LDS record of a texel is ONE binary32 value (+ the 16-byte analysis record): 20 B per texel where kEasuLdsPerTexel is 32;
//   * luma*2 of a texel, B*0.5 + (R*0.5 + G) (ffx_fsr1.h:363-366, RCAS :731-739), is 0.5 L + round(1.5 L) — not 2 L for every binary32
//     L — and is evaluated as the reference writes it (mono_luma2) where it is used, not stored;
//   * a window row of the 12 taps is four consecutive dwords, the filter accumulates one channel and the weight sum, the dering bounds
//     and RCAS's limiter exist once.
//
// Every global access is naturally aligned to its own width: a kernel takes an access of several elements only where its instantiation
// (WIDE) was chosen by a host that has checked base, pitch and frame stride against that width.
#pragma once
#include "fsr1_device_easu.hpp"
#include "fsr1_device_rcas.hpp"

namespace fsr1 {

// U: the bits of one element; load / store: an element to and from the filter's binary32.
template <int FMT> struct Mono;  // FMT = a single-channel fsr1_format
template <> struct Mono<FSR1_FORMAT_R16F> {
  typedef uint16_t U;
  static __device__ __forceinline__ float load(U u) { return (float)__builtin_bit_cast(half_t, u); }
  static __device__ __forceinline__ U store(float x) { return __builtin_bit_cast(U, (half_t)x); }  // RTNE, as Pixel<RGBA16F>::store
};
template <> struct Mono<FSR1_FORMAT_R32F> {
  typedef uint32_t U;
  static __device__ __forceinline__ float load(U u) { return as_f32(u); }
  static __device__ __forceinline__ U store(float x) { return as_u32(x); }
};
template <> struct Mono<FSR1_FORMAT_R8_UNORM> {  // 8-bit codes under the conversions pinned for RGBA8_UNORM (fsr1_hip.h)
  typedef uint8_t U;
  static __device__ __forceinline__ float load(U u) { return unorm_decode<255>(u); }
  static __device__ __forceinline__ U store(float x) { return (U)unorm_encode<255>(x); }
};

// luma*2 of the texel (L, L, L): the reference's expression, as easu_stage_footprint and rcas_pixel evaluate it
__device__ __forceinline__ float mono_luma2(float l) { return fmaf(l, 0.5f, fmaf(l, 0.5f, l)); }

// N dwords as one access (N = 1, 2, 4), aligned to their size
template <int N> struct Words { typedef uint32_t T __attribute__((ext_vector_type(N), aligned(4 * N))); };
template <> struct Words<1> { typedef uint32_t T; };

// G adjacent columns of a row, packed as in memory, in G * sizeof(U) / 4 dwords: what a lane of the RCAS strip kernel moves per row and
// keeps in its ring (uint8: four columns a register, decoded once, as Plane<RGB8_UNORM_PLANAR>).
template <int FMT, int G>
struct MonoGroup {
  typedef typename Mono<FMT>::U U;
  static constexpr int kPer = 4 / (int)sizeof(U), kWords = G / kPer;  // elements per dword, dwords
  static_assert(G % kPer == 0 && (kWords == 1 || kWords == 2 || kWords == 4), "a group is one access of 4, 8 or 16 bytes");
  typedef typename Words<kWords>::T V;
  uint32_t w[kWords];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < kWords; ++k) w[k] = 0u;
  }
  __device__ __forceinline__ void load_wide(const char* p) {
    const V v = *reinterpret_cast<const V*>(p);
    if constexpr (kWords == 1) {
      w[0] = v;
    } else {
#pragma unroll
      for (int k = 0; k < kWords; ++k) w[k] = v[k];
    }
  }
  // element i of the group: its bits, its value, and its replacement (i is a literal after unrolling at every call site)
  __device__ __forceinline__ U elem(int i) const { return (U)(w[i / kPer] >> (8 * (int)sizeof(U) * (i % kPer))); }
  __device__ __forceinline__ float get(int i) const { return Mono<FMT>::load(elem(i)); }
  __device__ __forceinline__ void put(int i, U u) {
    const int shift = 8 * (int)sizeof(U) * (i % kPer);
    if constexpr (kPer == 1) w[i] = u;
    else w[i / kPer] = (w[i / kPer] & ~((uint32_t)(U)~(U)0 << shift)) | ((uint32_t)u << shift);
  }
  // the stored form of G results
  static __device__ __forceinline__ MonoGroup pack(const float (&x)[G]) {
    MonoGroup g;
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
      if constexpr (FMT == FSR1_FORMAT_R16F) {  // one v_cvt_pk_f16_f32 (RTNE) per dword, as Pixel<RGBA16F>::store
        g.w[k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(float2_t{x[2 * k], x[2 * k + 1]}, half2_t));
      } else if constexpr (FMT == FSR1_FORMAT_R32F) {
        g.w[k] = as_u32(x[k]);
      } else {  // (codes are <= 255: nothing to mask)
        g.w[k] = unorm_encode<255>(x[4 * k]) | (unorm_encode<255>(x[4 * k + 1]) << 8) | (unorm_encode<255>(x[4 * k + 2]) << 16) | (unorm_encode<255>(x[4 * k + 3]) << 24);
      }
    }
    return g;
  }
  __device__ __forceinline__ void store_wide(char* p, bool streaming) const {
    V v;
    if constexpr (kWords == 1) {
      v = w[0];
    } else {
#pragma unroll
      for (int k = 0; k < kWords; ++k) v[k] = w[k];
    }
    store_out<sizeof(V)>(p, v, streaming);
  }
};

// ------------------------------------------------------------------------------------------------------------------------------
// EASU
// ------------------------------------------------------------------------------------------------------------------------------

// LDS bytes per footprint texel: the value + the analysis record
constexpr int kEasuMonoLdsPerTexel = 4 + 16;
// bytes of the staged footprint: the value plane rounded up to the analysis records' 16-byte alignment, then the records
__host__ __device__ constexpr size_t easu_mono_value_bytes(size_t capacity_texels) { return (capacity_texels * 4 + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t easu_mono_lds_region_bytes(size_t capacity_texels) { return easu_mono_value_bytes(capacity_texels) + capacity_texels * 16; }

struct EasuMonoLds {
  float* val;     // [n] the texel
  float4_t* ana;  // [n] FsrEasuSetF terms of the '+' around the texel, as EasuLds::ana
  int fw;         // row pitch of val / ana in texels (dense layout: the footprint width)
};
__device__ __forceinline__ EasuMonoLds easu_mono_lds_carve(char* smem, int capacity_texels) {
  return EasuMonoLds{reinterpret_cast<float*>(smem), reinterpret_cast<float4_t*>(smem + easu_mono_value_bytes((size_t)capacity_texels)), 0};
}

// Phases 1 and 2 of easu_stage_footprint for a single-channel input: the footprint [fx0, fx0 + fw) x [fy0, fy0 + fh) with the sampler's
// clamp-to-edge applied.  Phase 1 is easu_stage_footprint_planar's walk — one wave per footprint row, one lane per footprint column, the
// row base scalar, all of a wave's loads issued before the first conversion — with ONE element load per texel and one ds_write_b32 per
// texel whose 64 lanes fall into 64 different banks.  Phase 2 evaluates easu_analysis<EXACT> on the lumas of the '+' neighbourhood,
// each computed from its value by the reference's expression.  The five reads of a neighbourhood are ds_read_b32 of CONSECUTIVE dwords
// across the lanes of a footprint row (from the RGBA records they sit four dwords apart: 4-way bank conflicts, fsr1_device_easu.hpp) —
// conflict-free, except where a wave's 64 texels wrap from one footprint row to the next: each wrap skips the two border columns, so
// the wave's addresses span 66 - 68 dwords instead of 64 and two to four of its lanes share a bank with another (2-way, on those
// lanes only).  Ends with a barrier.  FW, FH: compile-time footprint extent (the exact-2x tiles), 0 = run-time.  Footprints wider than
// a wave (minification) take a linear walk.  All THREADS threads of the workgroup must make the call.
template <int FMT, bool EXACT, int FW = 0, int FH = 0, int THREADS = 256>
__device__ __forceinline__ void easu_stage_footprint_mono(const EasuMonoLds& l, const ImageView& in, const char* in_frame, int fx0, int fy0, int fw_rt,
                                                          int fh_rt, int tid) {
  typedef typename Mono<FMT>::U elem_t;
  const int fw = FW ? FW : fw_rt, fh = FH ? FH : fh_rt;
  if (FW || fw <= 64) {
    static_assert(FW <= 64 && THREADS % 64 == 0, "one lane per footprint column");
    constexpr int kWaves = THREADS / 64;
    constexpr int kU = FH ? (FH + kWaves - 1) / kWaves : 5;  // rows per wave and trip: kU element loads in flight per lane
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t xoff = (uint32_t)min(max(fx0 + lane, 0), in.width - 1) * (uint32_t)sizeof(elem_t);
    float* const rec = l.val + lane;
    if (lane < fw) {
#pragma unroll 1
      for (int ly0 = wave; ly0 < fh; ly0 += kWaves * kU) {
        elem_t px[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int ly = ly0 + kWaves * u;  // wave-uniform
          if (ly < fh) px[u] = *reinterpret_cast<const elem_t*>(in_frame + (long long)min(max(fy0 + ly, 0), in.height - 1) * in.pitch + (size_t)xoff);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int ly = ly0 + kWaves * u;
          if (ly < fh) rec[ly * fw] = Mono<FMT>::load(px[u]);
        }
      }
    }
  } else {
    const int n = fw * fh;
    const float inv_fw = __builtin_amdgcn_rcpf((float)fw);  // (i + 0.5) / fw lies 0.5 / fw from an integer: 1 ulp is plenty
    for (int i = tid; i < n; i += THREADS) {
      const int ly = (int)(((float)i + 0.5f) * inv_fw);
      const int gy = min(max(fy0 + ly, 0), in.height - 1), gx = min(max(fx0 + (i - ly * fw), 0), in.width - 1);
      l.val[i] = Mono<FMT>::load(*reinterpret_cast<const elem_t*>(in_frame + (long long)gy * in.pitch + (size_t)gx * sizeof(elem_t)));
    }
  }
  __syncthreads();
  // phase 2, as in easu_stage_footprint: FsrEasuSetF's terms for columns 1 .. fw - 2, rows 1 .. fh - 2 of the footprint
  const int iw = fw - 2, m = iw * (fh - 2);
  const float inv_iw = __builtin_amdgcn_rcpf((float)iw);
  for (int j = tid; j < m; j += THREADS) {
    const int y = FW ? j / (FW - 2) : (int)(((float)j + 0.5f) * inv_iw);
    const int i = (y + 1) * fw + (j - y * iw) + 1;
    l.ana[i] = easu_analysis<EXACT>(mono_luma2(l.val[i - fw]), mono_luma2(l.val[i - 1]), mono_luma2(l.val[i]), mono_luma2(l.val[i + 1]), mono_luma2(l.val[i + fw]));
  }
  __syncthreads();
}

// easu_filter on one channel: sub-texel position (ppx, yt), the 12-tap window through `tex(dx, dy)` -> value with (0, 0) the texel 'f',
// the four analyses through `ana(k)`.  Returns aC * rcp(aW) — channel R of easu_filter<EXACT> on the replicated window: the statements
// of that function (EXACT: the reference's operation order; default: easu_pixel_terms, easu_tap_weight and its tap order) with the two
// other accumulators left out.
template <bool EXACT, class Tex, class Ana>
__device__ __forceinline__ float easu_mono_filter(const Tex& tex, const Ana& ana, float ppx, const EasuRowTerms& yt) {
  const float oxm = -1.0f - ppx, ox0 = 0.0f - ppx, ox1 = 1.0f - ppx, ox2 = 2.0f - ppx;
  float aC, aW;
  if constexpr (EXACT) {
    const float ppy = yt.ppy;
    const float omx = 1.0f - ppx, omy = yt.omy;
    // :381-386 bilinear accumulation of the 4 analyses (f, g, j, k), reference order
    const float4_t af = ana(0), ag = ana(1), aj = ana(2), ak = ana(3);
    const float wS = omx * omy, wT = ppx * omy, wU = omx * ppy, wV = ppx * ppy;
    float dirx = af.x * wS;
    float diry = af.y * wS;
    dirx += ag.x * wT; diry += ag.y * wT;
    dirx += aj.x * wU; diry += aj.y * wU;
    dirx += ak.x * wV; diry += ak.y * wV;
    float len = af.z * wS;
    len = af.w * wS + len;
    len = ag.z * wT + len; len = ag.w * wT + len;
    len = aj.z * wU + len; len = aj.w * wU + len;
    len = ak.z * wV + len; len = ak.w * wV + len;
    // :389-395 normalise
    const float dir2x = dirx * dirx, dir2y = diry * diry;
    float dirR = dir2x + dir2y;
    const bool zro = dirR < (1.0f / 32768.0f);
    dirR = zro ? 1.0f : APrxLoRsqF1(dirR);
    dirx = zro ? 1.0f : dirx;
    dirx *= dirR;
    diry *= dirR;
    // :397-409 kernel shape
    len = len * 0.5f;
    len *= len;
    const float stretch = (dirx * dirx + diry * diry) * APrxLoRcpF1(fmaxf(fabsf(dirx), fabsf(diry)));
    const float len2x = (stretch - 1.0f) * len + 1.0f;
    const float len2y = -0.5f * len + 1.0f;
    const float lob = (float)((1.0 / 4.0 - 0.04) - 0.5) * len + 0.5f;
    const float clp = APrxLoRcpF1(lob);
    // :421-434 12 taps.  aC += c*w ; aW += w
    aC = 0.f;
    aW = 0.f;
    auto tap = [&](int dx, int dy, float offx, float offy) {
      const float c = tex(dx, dy);
      float vx = (offx * dirx) + (offy * diry);
      float vy = (offx * (-diry)) + (offy * dirx);
      vx *= len2x;
      vy *= len2y;
      float d2 = vx * vx + vy * vy;
      d2 = fminf(d2, clp);
      float wB = (float)(2.0 / 5.0) * d2 + -1.0f;
      float wA = lob * d2 + -1.0f;
      wB *= wB;
      wA *= wA;
      wB = (float)(25.0 / 16.0) * wB + (float)(-(25.0 / 16.0 - 1.0));
      const float w = wB * wA;
      aC += c * w;
      aW += w;
    };
    const float oym = yt.oym, oy0 = yt.oy0, oy1 = yt.omy, oy2 = yt.oy2;
    // reference order: b c i j f e k l h g o n
    tap(0, -1, ox0, oym); tap(1, -1, ox1, oym); tap(-1, 1, oxm, oy1); tap(0, 1, ox0, oy1);
    tap(0, 0, ox0, oy0); tap(-1, 0, oxm, oy0); tap(1, 1, ox1, oy1); tap(2, 1, ox2, oy1);
    tap(2, 0, ox2, oy0); tap(1, 0, ox1, oy0); tap(1, 2, ox1, oy2); tap(0, 2, ox0, oy2);
  } else {
    const EasuTapTerms h = easu_pixel_terms(ana, ppx, yt);
    auto tap = [&](int dx, int dy, float ox, float s, float b) {
      const float w = easu_tap_weight(h, ox, s, b);
      aC = fmaf(tex(dx, dy), w, aC);
      aW += w;
    };
    aW = easu_tap_weight(h, ox0, h.sm, h.bm);  // the first tap starts the sums
    aC = tex(0, -1) * aW;
    tap(1, -1, ox1, h.sm, h.bm);
    tap(-1, 0, oxm, h.s0, h.b0); tap(0, 0, ox0, h.s0, h.b0); tap(1, 0, ox1, h.s0, h.b0); tap(2, 0, ox2, h.s0, h.b0);
    tap(-1, 1, oxm, h.s1, h.b1); tap(0, 1, ox0, h.s1, h.b1); tap(1, 1, ox1, h.s1, h.b1); tap(2, 1, ox2, h.s1, h.b1);
    tap(0, 2, ox0, h.s2, h.b2); tap(1, 2, ox1, h.s2, h.b2);
  }
  const float rW = EXACT ? 1.0f / aW : __builtin_amdgcn_rcpf(aW);  // (as easu_filter)
  return pinned(aC * rW);
}

// The 12-tap window of the texel at footprint index f_idx, row by row: two, four, four and two ADJACENT dwords.  A lane's window
// starts at any dword (f_idx is a lane's own, the footprint pitch is odd at exactly 2x), so the reads cannot be ds_read_b64 / b128,
// which want 8 / 16-byte addresses: adjacent pairs are ds_read2_b32, which has no alignment beyond the dword — six instructions for the
// window, where the RGBA record form takes twelve ds_read_b128.  Index (dy + 1) * 4 + (dx + 1); the four corners are never read.
struct EasuMonoWindow {
  float v[16];
  __device__ __forceinline__ float operator()(int dx, int dy) const { return v[(dy + 1) * 4 + (dx + 1)]; }
};
__device__ __forceinline__ EasuMonoWindow easu_mono_window(const EasuMonoLds& l, int f_idx) {
  const int fw = l.fw;
  const float* const w0 = l.val + (f_idx - fw - 1);  // the window's top-left texel (-1, -1), as easu_pixel
  EasuMonoWindow w;
  w.v[1] = w0[1]; w.v[2] = w0[2];
  w.v[4] = w0[fw]; w.v[5] = w0[fw + 1]; w.v[6] = w0[fw + 2]; w.v[7] = w0[fw + 3];
  w.v[8] = w0[2 * fw]; w.v[9] = w0[2 * fw + 1]; w.v[10] = w0[2 * fw + 2]; w.v[11] = w0[2 * fw + 3];
  w.v[13] = w0[3 * fw + 1]; w.v[14] = w0[3 * fw + 2];
  return w;
}

// Dering bounds (:416-419) of the 2 x 2 block f g / j k of a window, and the clamp of easu_clamp on one channel (+ `c *= c`).
struct EasuMonoBounds { float mn, mx; };
__device__ __forceinline__ EasuMonoBounds easu_mono_bounds(const EasuMonoWindow& w) {
  return EasuMonoBounds{min4_asm(w(0, 0), w(1, 0), w(0, 1), w(1, 1)), max4_asm(w(0, 0), w(1, 0), w(0, 1), w(1, 1))};
}
template <bool EXACT>
__device__ __forceinline__ float easu_mono_clamp(const EasuMonoBounds& m, float p, bool hdr_square) {
  float c = EXACT ? fminf(m.mx, fmaxf(m.mn, p)) : __builtin_amdgcn_fmed3f(p, m.mn, m.mx);
  if (hdr_square) c *= c;
  return pinned(c);
}

// The filter for one pixel of a staged footprint: window and analyses from LDS, bounds of the window's values.
template <bool EXACT>
__device__ __forceinline__ float easu_mono_pixel(const EasuMonoLds& l, int f_idx, float ppx, const EasuRowTerms& yt, bool hdr_square) {
  const EasuMonoWindow w = easu_mono_window(l, f_idx);
  const float4_t* const a0 = l.ana + f_idx;
  const int fw = l.fw;
  const float p = easu_mono_filter<EXACT>(w, [&](int k) { return a0[(k >> 1) * fw + (k & 1)]; }, ppx, yt);
  return easu_mono_clamp<EXACT>(easu_mono_bounds(w), p, hdr_square);
}

__device__ __forceinline__ uint32_t dpp_shl1_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kDppWaveShl1, 0xf, 0xf, false); }

// A row of an exact-2x quad into the plane.  The quad's columns are {odd, even} (the tiles are shifted by one pixel), so the lane's own
// pair is not aligned to two elements.  The lane exchange of planar_store_quad_row was taken (the wave-local LDS run of the 3-channel
// kernel, rgb_store_run_rows, which would reach 8-16 bytes per lane: not built, unmeasured): WIDE, every lane takes the LEFT pixel of
// the lane to its right through one DPP move and stores the even-aligned pair {own right, neighbour's left} — 4 bytes (binary16) or
// 8 (binary32); the tile's first quad column stores its left pixel alone and the last one its right pixel alone.  8-bit: the pair
// would be two bytes, so each lane packs its two codes into one register, two DPP moves hand it the pairs of the next two lanes, and
// the EVEN quad columns store one dword — columns 64 tx + 2 qx .. + 3, a multiple of four; quad column 30 has three columns left in
// the tile and stores them, like a dword cut by the image's right edge, byte by byte.  So no store is narrower than 4 bytes except at
// a tile row's head and tail and at the image's right edge.  Every lane of the wave must make the call (the neighbours' values travel
// through it); `o` = address of the left pixel, column oxa (odd), W = image width, qx = quad column in the 32-quad tile row.
// WIDE = false: the two pixels element by element.
template <int FMT, bool WIDE>
__device__ __forceinline__ void mono_store_quad_row(char* o, float left, float right, int qx, int oxa, int W, bool row_in, bool streaming) {
  typedef typename Mono<FMT>::U elem_t;
  const bool xin0 = oxa >= 0 && oxa < W, xin1 = oxa + 1 < W;
  const elem_t l = Mono<FMT>::store(left), r = Mono<FMT>::store(right);
  if constexpr (!WIDE) {
    if (!row_in) return;
    if (xin0) store_out<sizeof(elem_t)>(o, l, streaming);
    if (xin1) store_out<sizeof(elem_t)>(o + sizeof(elem_t), r, streaming);
  } else if constexpr (FMT == FSR1_FORMAT_R8_UNORM) {
    const uint32_t own = (uint32_t)l | ((uint32_t)r << 8);
    const uint32_t n1 = dpp_shl1_u32(own), n2 = dpp_shl1_u32(n1);  // the pairs of the next two lanes
    if (!row_in || (qx & 1)) return;
    if (qx == 0 && xin0) store_out<1>(o, l, streaming);
    const int n = min(qx == 30 ? 3 : 4, W - (oxa + 1));  // columns oxa + 1 .. oxa + n are this lane's to store (n <= 0: none)
    const uint32_t quad = (uint32_t)r | ((n1 & 0xffffu) << 8) | (n2 << 24);  // {own right, next left, next right, next-but-one left}
    if (n == 4) {
      store_out<4>(o + 1, quad, streaming);
    } else {
      if (n > 0) store_out<1>(o + 1, (uint8_t)quad, streaming);
      if (n > 1) store_out<1>(o + 2, (uint8_t)(quad >> 8), streaming);
      if (n > 2) store_out<1>(o + 3, (uint8_t)(quad >> 16), streaming);
    }
  } else {
    typedef elem_t pair_t __attribute__((ext_vector_type(2), aligned(2 * sizeof(elem_t))));
    const elem_t nl = (elem_t)dpp_shl1_u32((uint32_t)l);
    if (!row_in) return;
    if (qx == 0 && xin0) store_out<sizeof(elem_t)>(o, l, streaming);
    if (qx < 31 && oxa + 2 < W) store_out<sizeof(pair_t)>(o + sizeof(elem_t), pair_t{r, nl}, streaming);
    else if (xin1) store_out<sizeof(elem_t)>(o + sizeof(elem_t), r, streaming);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// RCAS
// ------------------------------------------------------------------------------------------------------------------------------

// rcas_pixel on one channel: the 5 taps b above, d left, e centre, f right, h below.  Channel R of rcas_pixel<EXACT> on the replicated
// taps, bit for bit: the same operand order; max3(lobeR, lobeG, lobeB) of three equal lobes is that lobe, and the denoise lumas are
// the reference's expression of (L, L, L).
template <bool EXACT>
__device__ __forceinline__ float rcas_mono_pixel(float b, float d, float e, float f, float h, float sharp, uint32_t flags) {  // flags: compile-time 0 in the plain variant
  // :741-746 min and max of the ring (vmin3 / vmax3: the taps come from loop-carried registers and DPP moves, see rcas_pixel)
  const float mn4 = vmin2(vmin3(b, d, f), h), mx4 = vmax2(vmax3(b, d, f), h);
  // :748-755 limiters
  auto rcp = [](float x) { return EXACT ? rcp_ieee(x) : __builtin_amdgcn_rcpf(x); };
  const float hitMin = vmin2(mn4, e) * rcp(4.0f * mx4);
  const float hitMax = (1.0f - vmax2(mx4, e)) * rcp(fmaf(4.0f, mn4, -4.0f));
  // :756-759
  const float lobeC = fmaxf(-hitMin, hitMax);
  float lobe = fmaxf(-(0.25f - (1.0f / 16.0f)), fminf(lobeC, 0.0f)) * sharp;
  if (flags & FSR1_FLAG_RCAS_DENOISE) {  // :731-739, :761-763
    const float bL = mono_luma2(b), dL = mono_luma2(d), eL = mono_luma2(e), fL = mono_luma2(f), hL = mono_luma2(h);
    float nz = 0.25f * bL + 0.25f * dL + 0.25f * fL + 0.25f * hL - eL;
    nz = sat(fabsf(nz) * APrxMedRcpF1<EXACT>(max3f(max3f(bL, dL, eL), fL, hL) - min3f(min3f(bL, dL, eL), fL, hL)));
    nz = mad<EXACT>(-0.5f, nz, 1.0f);
    lobe *= nz;
  }
  // :765-768 resolve
  const float rcpL = APrxMedRcpF1<EXACT>(mad<EXACT>(4.0f, lobe, 1.0f));
  float p = EXACT ? (lobe * b + lobe * d + lobe * h + lobe * f + e) * rcpL : fmaf(lobe, (b + h) + (d + f), e) * rcpL;
  if (flags & FSR1_FLAG_HDR_SQUARE) p *= p;  // FSR_Pass.hlsl:92-93
  return pinned(p);
}

}  // namespace fsr1
