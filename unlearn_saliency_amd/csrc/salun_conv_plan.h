// salun_conv_plan.h - which kernel a call of the fp32 convolution family (salun_conv.hip) runs, on which tiles.
//
// A call is PLANNED by a pure function of its shape - no HIP call, no pointer: a pointer enters as "is 16-byte
// aligned", reduced to a boolean at the C-ABI entry - and then LAUNCHED from the plan (salun_conv.hip).  One plan per
// direction: plan_data (forward and stride-1 backward-data), plan_dgrad_s2, plan_wgrad.  salun_conv2d_route prints
// the plan the entry point would execute as a label, which is how tests/conv_routes.py is held to this file.
#pragma once
#include <cstddef>
#include <cstdio>
#include "../../include/salun.h"

// salun_conv_ring.hip: is this shape the LDS-DMA ring backward-weight kernel's (3x3 / stride 1 / pad 1 layers), for
// `nchunks` 64-pixel chunks and x, dy on 16-byte boundaries
bool salun_ring_wgrad_fits(int N, int C, int H, int W, int K, int nchunks, bool in_al16);

namespace {

constexpr int CC = 8;  // reduction channels staged per chunk
// conv_igemm's chunk: a 1x1 stride-1 convolution has one MFMA step per two channels, so an 8-channel chunk is four
// steps between two barrier pairs (72 TFLOP/s on the DDPM attention / skip projections); 32 channels make it sixteen.
constexpr int igemm_chunk(int R, int stride) { return (R == 1 && stride == 1) ? 32 : CC; }

// reduction channels per chunk of the rectangular-tap kernel (conv_dgrad_tap): 32 / taps, at least 8
constexpr int tap_chunk(int taps) { return taps == 1 ? 32 : taps == 2 ? 16 : 8; }

struct TileGeom {
  int NI, TP, IH_t, IW_t, logQ;
  int ntiles;
  bool ok;
  int psz() const { return NI * IH_t * IW_t; }  // floats of one channel's patch
};

inline int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// pixel tiling of an output of N x P x Q into tiles of `pixt` pixels; conv stride cs, RH x RW taps
inline TileGeom make_geom(int N, int P, int Q, int pixt, int cs, int RH, int RW) {
  TileGeom g{};
  g.ok = false;
  if (Q <= 0 || (Q & (Q - 1)) != 0 || Q > pixt) return g;  // Q power of two, at most one tile wide
  g.logQ = ilog2(Q);
  const int PQ = P * Q;
  if (PQ >= pixt) {
    if (PQ % pixt != 0) return g;
    g.NI = 1;
    g.TP = pixt / Q;
    g.ntiles = N * (PQ / pixt);
  } else {
    if (pixt % PQ != 0) return g;
    g.NI = pixt / PQ;
    g.TP = P;
    g.ntiles = (N + g.NI - 1) / g.NI;
  }
  g.IH_t = (g.TP - 1) * cs + RH;
  g.IW_t = (Q - 1) * cs + RW;
  g.ok = g.psz() <= 3 * 256;
  return g;
}
inline TileGeom make_geom(int N, int P, int Q, int pixt, int cs, int R) { return make_geom(N, P, Q, pixt, cs, R, R); }

// ---------------------------------------------------------------------------------------------------
// The workgroup tile of the data kernels: `pixt` pixels (PT 32-pixel tiles per wave, WP waves across) x WK*KT*32 channels.
struct Tile {
  TileGeom g;
  int pixt, KT, WP, WK, PT;
  int kb() const { return WK * KT * 32; }
};

// pixel tile: prefer 128 pixels; 64 when that is outside the tiling domain or leaves the chip under-filled (fewer than
// `need` workgroups over `blocks` channel blocks)
inline void pick_pixels(Tile &t, int N, int P, int Q, int blocks, int need, int cs, int RH, int RW) {
  t.pixt = 128;
  t.g = make_geom(N, P, Q, 128, cs, RH, RW);
  if (!t.g.ok || t.g.ntiles * blocks < need) {
    const TileGeom g64 = make_geom(N, P, Q, 64, cs, RH, RW);
    if (g64.ok) { t.g = g64; t.pixt = 64; }
  }
}

// tile shape of conv_igemm / conv_dgrad_tap: prefer 128 pixels x up to 128 channels; shrink when that leaves the chip
// under-filled (t.g.ok false: outside the tiling domain)
inline Tile pick_tile(int N, int yC, int P, int Q, int cs, int RH, int RW) {
  Tile t{};
  const int kblocks128 = (yC + 127) / 128;
  pick_pixels(t, N, P, Q, kblocks128, 384, cs, RH, RW);
  t.PT = 1;
  if (t.pixt == 128) {
    t.WP = 4; t.WK = 1;
    t.KT = yC > 64 ? 4 : yC > 32 ? 2 : 1;
  } else {
    // small pixel space (deep layers): 64 x 128 tiles only if that still yields enough workgroups; 64 x 64 is the only
    // tiling an under-filled launch ends up with (and the only one that splits its reduction)
    t.WP = 2; t.WK = 2;
    t.KT = (yC > 64 && t.g.ntiles * kblocks128 >= 384) ? 2 : 1;
  }
  return t;
}

// tile shape of conv_dgrad_s2 over the sub-grid P x Q: channel tile 64 or 128 (4*KT accumulators per wave: KT <= 2),
// whole channel tiles only (checked by the caller)
inline Tile pick_tile_s2(int N, int C, int P, int Q, int fp) {
  Tile t{};
  pick_pixels(t, N, P, Q, (C + 63) / 64, 256, 1, fp, fp);
  t.PT = 1;
  if (t.pixt == 128) {
    t.WP = 4; t.WK = 1;
    t.KT = (C % 64 == 0) ? 2 : 1;
  } else {
    t.WP = 2; t.WK = 2;
    t.KT = (C % 128 == 0 && t.g.ntiles * (C / 128) >= 256) ? 2 : 1;
  }
  return t;
}

inline int tile_label(char *buf, size_t n, const Tile &t) {
  if (t.PT == 2) return snprintf(buf, n, "256/PT2");
  if (t.pixt == 128) return snprintf(buf, n, "128/KT%d", t.KT);
  return snprintf(buf, n, "64/KT%dWK2", t.KT);
}

// LDS of a data kernel: [CC][patch | 1] + [KB][CC*RS + 1] floats
inline size_t data_lds_bytes(const Tile &t, int cc, int RS) {
  return sizeof(float) * ((size_t)cc * (t.g.psz() | 1) + (size_t)t.kb() * (cc * RS + 1));
}

// Reduction split for under-filled launches (the 4x4 level of the DDPM U-Net at batch 128 is 128 workgroups of
// 64 pixels x 64 channels: half the CUs idle, the rest with one workgroup and nothing to hide its staging behind):
// S workgroups per output tile, each over C/S reduction channels, partial images in the caller's workspace.
inline int igemm_split(int wgs, int xC, int chunk, size_t out_elems, int HW, size_t ws_bytes) {
  if (wgs > 256 || HW % 4 != 0 || out_elems % 4 != 0) return 1;
  int S = 512 / (wgs < 1 ? 1 : wgs);
  if (S > 8) S = 8;
  while (S > 1 && (xC % (S * chunk) != 0 || xC / S < 4 * chunk)) --S;  // equal shares, >= 4 chunks each
  while (S > 1 && (size_t)S * out_elems * sizeof(float) > ws_bytes) --S;
  return S < 1 ? 1 : S;
}

// ---- forward and stride-1 backward-data (conv_igemm).  x = the tensor the patch is read from, y = the one written.
struct DataPlan {
  int rc;  // SALUN_OK, or SALUN_EINVAL: the call is refused
  int R, stride;
  bool dgrad;
  Tile t;
  bool fast;         // FAST staging
  bool epi;          // per-image bias / full-size addend in the epilogue (EPI instantiations)
  int S;             // reduction split (1: none)
  bool hw_declined;  // an under-filled launch that may not split: the finishing kernel needs yH*yW % 4 == 0
  int wgs;           // workgroups of one reduction share
  size_t lds_bytes, out_elems;
};

inline DataPlan plan_data(int N, int xC, int yC, int yH, int yW, int R, int stride, bool dgrad, int wC, bool epi,
                          bool w_al16, bool split_al16, size_t ws_bytes) {
  DataPlan p{};
  p.rc = SALUN_EINVAL;
  p.R = R; p.stride = stride; p.dgrad = dgrad; p.epi = epi; p.S = 1;
  if (N < 1 || xC < 1 || yC < 1 || yH < 1 || yW < 1 || (R != 1 && R != 3) || (stride != 1 && stride != 2) ||
      (dgrad && stride != 1))
    return p;
  const int cs = dgrad ? 1 : stride, RS = R * R, CC = igemm_chunk(R, stride);
  p.t = pick_tile(N, yC, yH, yW, cs, R, R);
  if (!p.t.g.ok) return p;
  // FAST staging: full reduction chunks, channel tile inside the tensor, float4-aligned weight runs
  auto fast = [&](int KB) { return (xC % CC == 0) && (!dgrad || yC % KB == 0) && w_al16 && ((wC * RS) % 4 == 0); };
  if (p.t.pixt == 128 && p.t.KT == 2 && !epi) {
    // 64 output channels: a wave takes 64 pixels x 64 channels (PT = 2) when 256-pixel tiles still fill the chip
    // and the stride-1 fast path applies
    const TileGeom g256 = make_geom(N, yH, yW, 256, cs, R);
    if (g256.ok && fast(64) && g256.ntiles >= 512) { p.t.g = g256; p.t.pixt = 256; p.t.PT = 2; }
  }
  p.fast = fast(p.t.kb());
  if (epi && (!p.fast || dgrad || stride != 1)) return p;  // epilogue terms: stride-1 forward, FAST
  p.out_elems = (size_t)N * yC * yH * yW;
  p.wgs = p.t.g.ntiles * ((yC + p.t.kb() - 1) / p.t.kb());
  if (p.fast && p.t.pixt == 64 && p.t.KT == 1) {
    // the finishing kernel reads / writes y, the addends and the partials as float4: 16-byte bases or no split
    if (split_al16 && ws_bytes > 0) p.S = igemm_split(p.wgs, xC, CC, p.out_elems, yH * yW, ws_bytes);
    p.hw_declined = p.wgs <= 256 && (yH * yW) % 4 != 0;
  }
  p.lds_bytes = data_lds_bytes(p.t, CC, RS);
  p.rc = SALUN_OK;
  return p;
}

inline int data_label(char *buf, size_t n, const DataPlan &p) {
  char tile[16];
  tile_label(tile, sizeof tile, p.t);
  return snprintf(buf, n, "igemm<%d,%d%s>/%s/%s/S%d%s%s", p.R, p.stride, p.dgrad ? ",dgrad" : "", tile,
                  p.fast ? "fast" : "slow", p.S, p.hw_declined ? "/hw-declined" : "", p.epi ? "/epi" : "");
}

// ---- backward-data of a stride-2 convolution: conv_dgrad_s2 (all parity classes in one launch), or one conv_dgrad_tap
// launch per parity class for shapes outside its staging assumptions
struct TapClass {
  int RH, RW, ph, pw;                      // taps that reach output parity (ph, pw)
  int rtop_h, rtop_w, vpad_h, vpad_w;      // largest tap per dimension; patch origin
  Tile t;
  int maxpos;                              // conv_dgrad_tap's MAXPOS: 1 (patch <= 256 floats) or 3
  size_t lds_bytes;
};
struct Dgrad2Plan {
  int rc;
  int R, pad;
  bool merged;
  Tile t;            // merged
  size_t lds_bytes;  // merged
  int ncls;          // per class: the classes that receive a tap, in launch order
  TapClass cls[4];
  bool any_empty;    // a class no tap reaches: dx is first set to 0, or to the addend
};

inline Dgrad2Plan plan_dgrad_s2(int N, int C, int H, int W, int K, int R, int pad, int P, int Q, bool w_al16,
                                bool out_al16 /*dx and the addend: float2 row pairs*/) {
  Dgrad2Plan p{};
  p.rc = SALUN_EINVAL;
  p.R = R; p.pad = pad;
  if (N < 1 || C < 1 || K < 1 || P < 1 || Q < 1 || (R != 1 && R != 3) || (H & 1) || (W & 1)) return p;
  const int RS = R * R;
  if (H == 2 * P && W == 2 * Q && ((R == 3 && (pad == 0 || pad == 1)) || (R == 1 && pad == 0)) && K % CC == 0 &&
      w_al16 && (C * RS) % 4 == 0 && out_al16) {
    p.t = pick_tile_s2(N, C, P, Q, (R == 1) ? 1 : 2);
    if (p.t.g.ok && p.t.g.psz() <= 256 && C % p.t.kb() == 0) {
      p.merged = true;
      p.lds_bytes = data_lds_bytes(p.t, CC, RS);
      p.rc = SALUN_OK;
      return p;
    }
  }
  // taps of parity class q: r = (q + pad) mod 2, +2, ... < R ; rtop = the largest
  int ntap[2], rtop[2];
  for (int q = 0; q < 2; ++q) {
    const int r0 = (q + pad) & 1;
    ntap[q] = (r0 < R) ? (R - 1 - r0) / 2 + 1 : 0;
    rtop[q] = r0 + 2 * (ntap[q] - 1);
  }
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      if (ntap[ph] == 0 || ntap[pw] == 0) { p.any_empty = true; continue; }
      TapClass &c = p.cls[p.ncls++];
      c.RH = ntap[ph]; c.RW = ntap[pw]; c.ph = ph; c.pw = pw;
      c.rtop_h = rtop[ph]; c.rtop_w = rtop[pw];
      c.vpad_h = -((ph + pad - rtop[ph]) / 2);  // (ph + pad - rtop) is even and <= 0
      c.vpad_w = -((pw + pad - rtop[pw]) / 2);
      c.t = pick_tile(N, C, H / 2, W / 2, 1, c.RH, c.RW);
      if (!c.t.g.ok) return p;
      c.maxpos = c.t.g.psz() <= 256 ? 1 : 3;
      const int cct = tap_chunk(c.RH * c.RW);
      c.lds_bytes = data_lds_bytes(c.t, cct, c.RH * c.RW);
    }
  p.rc = SALUN_OK;
  return p;
}

inline int dgrad2_label(char *buf, size_t n, const Dgrad2Plan &p) {
  char tile[16];
  if (p.merged) {
    tile_label(tile, sizeof tile, p.t);
    return snprintf(buf, n, "dgrad_s2<%d,pad%d>/%s", p.R, p.pad, tile);
  }
  size_t o = (size_t)snprintf(buf, n, "dgrad_tap[");
  for (int i = 0; i < p.ncls && o < n; ++i) {
    const TapClass &c = p.cls[i];
    tile_label(tile, sizeof tile, c.t);
    o += (size_t)snprintf(buf + o, n - o, "%s<%d,%d>/%s%s", i ? " " : "", c.RH, c.RW, tile, c.maxpos == 3 ? "/P3" : "");
  }
  if (o < n) o += (size_t)snprintf(buf + o, n - o, "]%s", p.any_empty ? "/empty" : "");
  return (int)o;
}

// ---- backward-weight
// 1x1 (conv_wgrad_1x1): geometry and split count; 0 chunks = shape outside its domain
inline int wgrad1x1_chunks(int N, int P, int Q, int stride) {
  const int PQ = P * Q;
  if (PQ % 4 != 0 || (stride == 2 && Q % 4 != 0)) return 0;
  if (PQ >= 64) return (PQ % 64 == 0) ? N * (PQ / 64) : 0;
  return (64 % PQ == 0) ? (N + 64 / PQ - 1) / (64 / PQ) : 0;
}
inline int wgrad1x1_nsplit(int K, int C, int nchunks) {
  const int tiles = ((K + 127) / 128) * ((C + 127) / 128);
  int ns = (256 + tiles - 1) / tiles;
  if (ns > nchunks) ns = nchunks;
  return ns < 1 ? 1 : ns;
}

inline int wgrad_nsplit(int K, int C, int nchunks) {
  const int tiles = ((K + 63) / 64) * ((C + 63) / 64);
  // one workgroup per CU is resident (register budget): a single full round of 256 workgroups, each with a long
  // run of chunks, beats more and shorter splits (prologue/epilogue and partial-sum traffic scale with nsplit)
  // (round 5 sweep on the ResNet-18 step, profiles/r05_wgrad_sweep.txt: 128 / 192 / 256 / 384 / 512 target workgroups
  // -> 94.4 / 107.3 / 114.7 / 103.4 / 106.1 steps/s)
  int ns = (256 + tiles - 1) / tiles;
  if (ns > nchunks) ns = nchunks;
  if (ns < 1) ns = 1;
  return ns;
}

// small-C kernel (conv_wgrad_smallc): up to 1024 workgroups, each writing 2 pixel halves
inline int wgrad_smallc_nsplit(int K, int nchunks) {
  int ns = 1024 / ((K + 63) / 64);
  if (ns > nchunks) ns = nchunks;
  return ns < 1 ? 1 : ns;
}
inline bool wgrad_is_smallc(int C, int R) { return C * R * R <= 32 && C <= 4; }

enum WgradRoute { WG_1X1, WG_SMALLC, WG_RING, WG_V, WG_GENERAL };
struct WgradPlan {
  int rc;  // SALUN_OK, SALUN_EINVAL (outside the domain) or SALUN_ENOSPC (workspace below part_bytes)
  WgradRoute route;
  int R, stride, W;
  bool fullC;         // WG_GENERAL: C a multiple of 64
  int nit;            // WG_V: conv_wgrad_v's NIT
  int nchunks;        // pixel chunks of the batch
  int gz;             // grid.z: workgroups along the pixel range
  int nsplit;         // partial images the reduce kernel adds (2 per workgroup for WG_SMALLC)
  size_t part_bytes;  // of the workspace
  size_t lds_bytes;
  TileGeom g;
};

inline WgradPlan plan_wgrad(int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q, bool shared,
                            bool in_al16 /*x and dy*/, size_t ws_bytes) {
  WgradPlan p{};
  p.rc = SALUN_EINVAL;
  p.R = R; p.stride = stride; p.W = W;
  if (N < 1 || C < 1 || K < 1 || P < 1 || Q < 1) return p;
  if (!((R == 3 || R == 1) && (stride == 1 || stride == 2))) return p;
  const int RS = R * R;
  auto sized = [&](WgradRoute route, int gz, int nsplit) {  // route found: the call stands or falls with the workspace
    p.route = route; p.gz = gz; p.nsplit = nsplit;
    p.part_bytes = sizeof(float) * (size_t)nsplit * K * C * RS;
    p.rc = ws_bytes < p.part_bytes ? SALUN_ENOSPC : SALUN_OK;
  };
  if (R == 1 && pad == 0 && C >= 32 && H == P * stride && W == Q * stride && W % 4 == 0 && in_al16 &&
      (size_t)64 * C * H * W < (1u << 30) && (size_t)64 * K * P * Q < (1u << 30)) {
    p.nchunks = wgrad1x1_chunks(N, P, Q, stride);
    if (p.nchunks > 0) {  // GEMM-shaped 1x1 kernel
      const int ns = wgrad1x1_nsplit(K, C, p.nchunks);
      p.lds_bytes = sizeof(float) * 2 * 2 * 128 * 65;
      sized(WG_1X1, ns, ns);
      return p;
    }
  }
  const int pixc = (stride == 1) ? 64 : 32;
  p.g = make_geom(N, P, Q, pixc, stride, R);
  if (!p.g.ok || p.g.psz() > 256) return p;
  const TileGeom &g = p.g;
  p.nchunks = g.ntiles;
  const bool shifts = Q >= 4 && (g.TP & (g.TP - 1)) == 0;  // float4 dy staging; shift-only pixel decoding
  if (wgrad_is_smallc(C, R) && shifts) {  // RGB stem: columns = (c, r, s)
    const int ns = wgrad_smallc_nsplit(K, g.ntiles);
    p.lds_bytes = sizeof(float) * ((size_t)C * (g.psz() | 1) + (size_t)64 * (pixc + 1));
    sized(WG_SMALLC, ns, ns * 2);
    return p;
  }
  const int ns = wgrad_nsplit(K, C, g.ntiles);
  sized(WG_GENERAL, ns, ns);
  if (p.rc != SALUN_OK) return p;
  p.rc = SALUN_EINVAL;
  if (!shifts) return p;
  p.lds_bytes = sizeof(float) * 2 * ((size_t)64 * (g.psz() | 1) + (size_t)64 * (pixc + 1) + 256);  // double buffered
  // per-lane offsets inside one chunk's image block are 32-bit
  if ((size_t)g.NI * C * H * W >= (1u << 30) || (size_t)g.NI * K * P * Q >= (1u << 30)) return p;
  if (p.lds_bytes > 160 * 1024) return p;
  p.rc = SALUN_OK;
  p.fullC = C % 64 == 0;
  // 3x3 / stride 1 / pad 1 on square images: the LDS-DMA ring kernel (salun_conv_ring.hip)
  // ... unless the caller says the launch shares the device with another stream's kernels (SALUN_WGRAD_SHARED): beside a
  // second matrix kernel or a BatchNorm pass on the same SIMDs the ring kernel's dense MFMA stream buys nothing and costs
  // its neighbours more than conv_wgrad_v's does (round 6: ResNet-18 step 117.5 vs 116.1 steps/s, DDPM 9.59 vs 9.46 with
  // backward-weight on the side stream; alone it is 12 - 18 % faster, and the single-stream step 111.8 vs 107.9)
  if (R == 3 && stride == 1 && pad == 1 && P == H && Q == W && !shared &&
      salun_ring_wgrad_fits(N, C, H, W, K, g.ntiles, in_al16)) {
    p.route = WG_RING;
    return p;
  }
  // vectorised staging (conv_wgrad_v) where the geometry allows it: 3x3, pad 1, full channel tiles, whole image rows
  if (R == 3 && pad == 1 && p.fullC && W % 4 == 0 && Q * stride == W && P * stride == H && in_al16 &&
      (size_t)g.NI * C * H * W < (1u << 30)) {
    const int F4C = g.NI * g.IH_t * (W / 4);
    const int nit = (F4C % 4 == 0) ? F4C / 4 : 0;
    if (stride == 1 ? (nit == 5 || nit == 6 || nit == 8) : (nit == 9 || nit == 10)) {
      p.route = WG_V;
      p.nit = nit;
    }
  }
  return p;
}

inline int wgrad_label(char *buf, size_t n, const WgradPlan &p) {
  switch (p.route) {
    case WG_1X1: return snprintf(buf, n, "wgrad_1x1<%d>", p.stride);
    case WG_SMALLC: return snprintf(buf, n, "wgrad_smallc<%d,%d>", p.R, p.stride);
    case WG_RING: return snprintf(buf, n, "wgrad_ring<W%d>", p.W);
    case WG_V: return snprintf(buf, n, "wgrad_v<%d,%d>", p.stride, p.nit);
    default: return snprintf(buf, n, "wgrad<%d,%d,%s>", p.R, p.stride, p.fullC ? "true" : "false");
  }
}

}  // namespace
