// tile_bins.h — the tile binner of the overlays that walk primitives (draw.cpp, redact.cpp): DrawPrims, added frame by frame in order,
// become the non-empty DrawTiles of every frame and the tiles' stretches of `index`, as draw_kernel and redact_kernel read them
// (kernels.h).  Plain host C++: kernels.h and the standard library only, so tools/probes/tile_bins_check.cpp checks it without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"

namespace dc {

struct __attribute__((visibility("hidden"))) TileBins {  // the library exports nothing of it
  std::vector<DrawPrim> prims;  // the primitives that reach a frame, in the order they were added
  std::vector<DrawTile> tiles;  // the non-empty tiles: by frame, then row, then column
  std::vector<int> index;       // every tile's primitives (places in `prims`), ascending
  std::vector<char> touched;    // [nb]: the frame has a tile

  TileBins(int nb, int h, int w)
      : touched((size_t)nb, 0), h_(h), w_(w), tiles_x_((w + kDrawTileW - 1) / kDrawTileW), count_((size_t)tiles_x_ * ((h + kDrawTileH - 1) / kDrawTileH)) {}

  // A primitive of the frame at hand.  It goes into every tile that holds a pixel CENTRE of its bounding box grown by the radius:
  // conservative, and the kernels' results do not depend on it (a tile's extra primitives cover none of its pixels).  -> whether there
  // is such a pixel in the frame; a primitive wholly outside is dropped
  bool add(const DrawPrim& p) {
    auto lo_px = [](int lo) { return (int)std::floor((lo - 8 + 15) / 16.0); };  // the first pixel whose centre 16 px + 8 is >= lo
    auto hi_px = [](int hi) { return (int)std::floor((hi - 8) / 16.0); };       // the last one whose centre is <= hi
    const int x0 = std::max(0, lo_px(std::min(p.ax, p.bx) - p.r16)), x1 = std::min(w_ - 1, hi_px(std::max(p.ax, p.bx) + p.r16));
    const int y0 = std::max(0, lo_px(std::min(p.ay, p.by) - p.r16)), y1 = std::min(h_ - 1, hi_px(std::max(p.ay, p.by) + p.r16));
    if (x0 > x1 || y0 > y1) return false;
    prims.push_back(p);
    bin(x0, y0, x1, y1);
    return true;
  }

  // A primitive of the frame at hand that is not a DrawPrim (a label: label.cpp), by the pixels [x0, x1] x [y0, y1] it may write, both
  // ends inclusive.  Nothing goes into `prims`: the caller keeps its own list, and `index` names places in it, counted over the boxes
  // added.  One binner takes either add or add_box, never both.  -> whether a pixel of the box lies in the frame
  bool add_box(int x0, int y0, int x1, int y1) {
    x0 = std::max(0, x0), y0 = std::max(0, y0), x1 = std::min(w_ - 1, x1), y1 = std::min(h_ - 1, y1);
    if (x0 > x1 || y0 > y1) return false;
    bin(x0, y0, x1, y1);
    return true;
  }

  // Frame b is complete: its non-empty tiles, row by row, each with its stretch of `index`; then the primitives in order fill the
  // stretches.  -> false once there are more than 2^30 primitive-tile pairs (the caller refuses; the binner is not used further)
  bool close_frame(int b) {
    const size_t first_prim = added_ - boxes_.size();
    if (boxes_.empty()) return true;
    touched[(size_t)b] = 1;
    slot_.assign(count_.size(), -1);
    for (size_t at = 0; at < count_.size(); ++at) {
      int& c = count_[at];
      if (!c) continue;
      slot_[at] = (int)tiles.size();
      tiles.push_back(DrawTile{b, (int)(at % (size_t)tiles_x_), (int)(at / (size_t)tiles_x_), (int)index.size(), 0});
      index.resize(index.size() + (size_t)c);
      if (index.size() > ((size_t)1 << 30)) return false;
      c = 0;  // ready for the next frame
    }
    for (size_t i = 0; i < boxes_.size(); ++i)
      for (int ty = boxes_[i].ty0; ty <= boxes_[i].ty1; ++ty)
        for (int tx = boxes_[i].tx0; tx <= boxes_[i].tx1; ++tx) {
          DrawTile& t = tiles[(size_t)slot_[(size_t)ty * tiles_x_ + tx]];
          index[(size_t)t.first + t.count++] = (int)(first_prim + i);
        }
    boxes_.clear();
    return true;
  }

  // What the kernels are given, as one block: tiles | index | prims, each rounded up to 256 bytes (frame_up, kernels.h)
  size_t index_at() const { return frame_up(tiles.size() * sizeof(DrawTile)); }
  size_t prims_at() const { return index_at() + frame_up(index.size() * sizeof(int)); }
  size_t bytes() const { return prims_at() + frame_up(prims.size() * sizeof(DrawPrim)); }
  void pack(unsigned char* to) const {
    std::memcpy(to, tiles.data(), tiles.size() * sizeof(DrawTile));
    std::memcpy(to + index_at(), index.data(), index.size() * sizeof(int));
    std::memcpy(to + prims_at(), prims.data(), prims.size() * sizeof(DrawPrim));
  }

 private:
  struct Box {
    int tx0, ty0, tx1, ty1;  // the tiles a primitive is binned into, inclusive
  };
  void bin(int x0, int y0, int x1, int y1) {  // in-frame pixels, inclusive
    const Box bx{x0 / kDrawTileW, y0 / kDrawTileH, x1 / kDrawTileW, y1 / kDrawTileH};
    boxes_.push_back(bx);
    ++added_;
    for (int ty = bx.ty0; ty <= bx.ty1; ++ty)
      for (int tx = bx.tx0; tx <= bx.tx1; ++tx) ++count_[(size_t)ty * tiles_x_ + tx];
  }
  size_t added_ = 0;               // primitives binned so far, over all frames
  int h_, w_, tiles_x_;
  std::vector<int> count_, slot_;  // per tile of the frame at hand: its primitives, then its place in `tiles`
  std::vector<Box> boxes_;         // of the frame at hand's primitives
};

}  // namespace dc
