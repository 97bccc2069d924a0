// label_tile.h — what the label overlay's code shares (the rule: include/deepcut_hip.h, dc_label_people).  The integer half of making a
// label — the key's digits, the anchor, the clamp — is one host-and-device function each, so label.cpp and the device builder
// (overlay.hip) cannot drift apart; what a tile does with a chunk of labels in LDS is shared by the kernel that is handed bins
// (label.hip) and the one that bins for itself (overlay.hip).  Integer only: no floating point, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "frame_tile.h"
#include "kernels.h"
#include "label_font.h"

namespace dc {

// ---- making a label ----------------------------------------------------------------------------------------------------------------------
// key >= 0 in decimal behind text[0 .. n) -> the new length: at most 19 digits more (2^63 - 1 has 19)
__host__ __device__ inline int label_put_key(long long key, unsigned char* text, int n) {
  unsigned char d[20];
  int nd = 0;
  do d[nd++] = (unsigned char)(key % 10), key /= 10;  // '0' .. '9' are places 0 .. 9 of the table
  while (key > 0);
  while (nd > 0) text[n++] = d[--nd];
  return n;
}

// The plate's size for n characters at scale s
__host__ __device__ inline int label_plate_w(int n, int s) { return s * (kLabelAdvance * n - 1) + 2 * s; }
__host__ __device__ inline int label_plate_h(int s) { return kLabelGlyphRows * s + 2 * s; }

// The held joints (qx, qy)[j] in 1/16 pixel, bit j of `held`, -> the plate's upper left pixel (X, Y), clamped; false without a held joint.
// anchor: -1, or a joint whose snapped place centres the label when it is held; else the upper left of the held joints' bounding box
__host__ __device__ inline bool label_place(const int* qx, const int* qy, unsigned held, int J, int anchor, int n, int s, int gap, int H, int W,
                                            int& X, int& Y) {
  if (!held) return false;
  const int pw = label_plate_w(n, s), ph = label_plate_h(s);
  int Yb;
  if (anchor >= 0 && anchor < J && (held >> anchor & 1u)) {
    X = (qx[anchor] >> 4) - (pw >> 1), Yb = qy[anchor] >> 4;  // >> is arithmetic
  } else {
    int lo_x = 0, lo_y = 0;
    bool first = true;
    for (int j = 0; j < J; ++j) {
      if (!(held >> j & 1u)) continue;
      lo_x = first ? qx[j] : (qx[j] < lo_x ? qx[j] : lo_x), lo_y = first ? qy[j] : (qy[j] < lo_y ? qy[j] : lo_y);
      first = false;
    }
    X = lo_x >> 4, Yb = lo_y >> 4;
  }
  Y = Yb - gap - ph;
  const int hi_x = W - pw > 0 ? W - pw : 0, hi_y = H - ph > 0 ? H - ph : 0;
  X = X < 0 ? 0 : (X > hi_x ? hi_x : X), Y = Y < 0 ? 0 : (Y > hi_y ? hi_y : Y);
  return true;
}

#ifdef __HIPCC__
// ---- the tile code -----------------------------------------------------------------------------------------------------------------------
// the kernels' copy of the font (label_font.h): staged into LDS once per workgroup
static __device__ const unsigned char kLabelFontDev[kLabelGlyphs][kLabelGlyphRows] = {DC_LABEL_FONT_ROWS};

// font[kLabelFontBytes] (LDS).  Every thread of the workgroup calls it; a barrier follows in the caller before the first read
__device__ __forceinline__ void label_stage_font(unsigned char* font) {
  for (int i = threadIdx.x; i < kLabelFontBytes; i += blockDim.x) font[i] = kLabelFontDev[i / kLabelGlyphRows][i % kLabelGlyphRows];
}

// the label reaches tile (tx, ty) of an H x W frame: its plate rectangle, clipped to the frame, holds a pixel of the tile
__device__ __forceinline__ bool label_reaches(const LabelPrim& p, int tx, int ty, int H, int W) {
  const int x1 = min(W - 1, p.x + label_plate_w(p.n, p.s) - 1), y1 = min(H - 1, p.y + label_plate_h(p.s) - 1);
  return p.x / kDrawTileW <= tx && tx <= x1 / kDrawTileW && p.y / kDrawTileH <= ty && ty <= y1 / kDrawTileH;
}

// The label rule on sp[0 .. m), in order, for the thread's block: per label the plate layer, then the text layer; the chroma sample
// once per layer, by the share of the block's in-frame pixels that layer covers
template <int FMT>
__device__ __forceinline__ void label_chunk(BlockPixels<FMT>& px, const LabelPrim* sp, int m, const unsigned char* font) {
  for (int i = 0; i < m; ++i) {
    const LabelPrim* p = sp + i;  // LDS, the same address in every lane
    const int X = p->x, Y = p->y, s = p->s, n = p->n;
    const int pw = label_plate_w(n, s), ph = label_plate_h(s);
    if (px.x0 + 1 < X || px.x0 >= X + pw || px.y0 + 1 < Y || px.y0 >= Y + ph) continue;  // the block lies outside the plate rectangle
    const int at = p->alpha_text, ap = p->alpha_plate;
    if (ap > 0) {
      const unsigned colour = p->plate_colour;
      int k = 0;
      for (int q = 0; q < 4; ++q) {
        const int x = px.x0 + (q & 1) - X, y = px.y0 + (q >> 1) - Y;
        if (!px.in[q] || x < 0 || x >= pw || y < 0 || y >= ph) continue;
        ++k;
        px.blend_pixel(q, colour, ap);
      }
      if (FMT == kFmtNv12 && k) px.blend_chroma(colour, (ap * k + px.n_in / 2) / px.n_in);
    }
    if (at > 0) {
      const unsigned colour = p->text_colour;
      const int tw = pw - 2 * s, th = ph - 2 * s;
      int k = 0;
      for (int q = 0; q < 4; ++q) {
        const int u = px.x0 + (q & 1) - X - s, v = px.y0 + (q >> 1) - Y - s;
        if (!px.in[q] || u < 0 || u >= tw || v < 0 || v >= th) continue;
        const int col = u / s, ch = col / kLabelAdvance, c = col % kLabelAdvance, r = v / s;
        if (c >= kLabelGlyphCols || !(font[(int)p->text[ch] * kLabelGlyphRows + r] >> (kLabelGlyphCols - 1 - c) & 1)) continue;
        ++k;
        px.blend_pixel(q, colour, at);
      }
      if (FMT == kFmtNv12 && k) px.blend_chroma(colour, (at * k + px.n_in / 2) / px.n_in);
    }
  }
}
#endif  // __HIPCC__

}  // namespace dc
