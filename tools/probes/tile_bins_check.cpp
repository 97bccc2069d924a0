// tile_bins_check.cpp — the tile binner of the overlays (deepcut-cnn_amd/csrc/tile_bins.h) against brute force, on the host alone:
// a few hundred seeded random discs and capsules go into three 70 x 45 frames (3 x 2 tiles, the last column and row partial; frame 1
// gets nothing; some primitives lie wholly outside, some span every tile, some have radius 1), and every tile of every frame is
// compared with what a walk over its pixels says.  Exits non-zero at the first mismatch.  Built by tests/test_tile_bins_host.py with
// -fsanitize=address,undefined.
//
//    g++ -std=c++17 -I deepcut-cnn_amd/csrc tools/probes/tile_bins_check.cpp -o tile_bins_check && ./tile_bins_check [seed]
#include <cstdio>
#include <cstdlib>
#include <random>

#include "tile_bins.h"

using namespace dc;

namespace {
constexpr int kFrames = 3, kH = 45, kW = 70;
constexpr int kTilesX = (kW + kDrawTileW - 1) / kDrawTileW, kTilesY = (kH + kDrawTileH - 1) / kDrawTileH;

#define EXPECT(cond, ...)                          \
  do {                                             \
    if (!(cond)) {                                 \
      std::fprintf(stderr, "MISMATCH: " __VA_ARGS__); \
      std::fprintf(stderr, "  (%s)\n", #cond);     \
      std::exit(1);                                \
    }                                              \
  } while (0)

// the centre of pixel (x, y), 16 x + 8, lies in the primitive's box grown by its radius — integers only, no rounding
bool centre_in_box(const DrawPrim& p, int x, int y) {
  const int cx = 16 * x + 8, cy = 16 * y + 8;
  return cx >= std::min(p.ax, p.bx) - p.r16 && cx <= std::max(p.ax, p.bx) + p.r16 && cy >= std::min(p.ay, p.by) - p.r16 &&
         cy <= std::max(p.ay, p.by) + p.r16;
}
bool tile_holds(const DrawPrim& p, int tx, int ty) {
  for (int y = ty * kDrawTileH; y < std::min(kH, (ty + 1) * kDrawTileH); ++y)
    for (int x = tx * kDrawTileW; x < std::min(kW, (tx + 1) * kDrawTileW); ++x)
      if (centre_in_box(p, x, y)) return true;
  return false;
}
bool same(const DrawPrim& a, const DrawPrim& b) {
  return a.ax == b.ax && a.ay == b.ay && a.bx == b.bx && a.by == b.by && a.r16 == b.r16 && a.capsule == b.capsule && a.alpha == b.alpha &&
         a.colour == b.colour;
}
}  // namespace

int main(int argc, char** argv) {
  std::mt19937 rng(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
  auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  static_assert(kTilesX == 3 && kTilesY == 2, "3 x 2 tiles, the last column and row partial");

  TileBins bins(kFrames, kH, kW);
  std::vector<DrawPrim> given[kFrames];  // everything that was added, per frame
  std::vector<char> kept[kFrames];       // what add() answered
  int n_outside = 0, n_everywhere = 0, n_radius1 = 0;
  for (int b = 0; b < kFrames; ++b) {
    const int n = b == 1 ? 0 : 200;
    for (int i = 0; i < n; ++i) {
      DrawPrim p{};
      const int kind = i % 8;
      p.capsule = pick(0, 1);
      p.r16 = kind == 0 ? 1 : pick(1, 160);
      p.ax = pick(-16 * 20, 16 * (kW + 20)), p.ay = pick(-16 * 20, 16 * (kH + 20));
      if (kind == 0) p.ax = 16 * pick(0, kW - 1) + 8 + pick(-2, 2), p.ay = 16 * pick(0, kH - 1) + 8 + pick(-2, 2);  // at a pixel centre, or just off it
      if (kind == 1) p.ax = pick(0, 1) ? -16 * pick(30, 60) : 16 * (kW + pick(30, 60));  // wholly outside, left or right
      if (kind == 2) p.ay = pick(0, 1) ? -16 * pick(30, 60) : 16 * (kH + pick(30, 60));  // wholly outside, above or below
      p.bx = p.capsule ? p.ax + pick(-300, 300) : p.ax, p.by = p.capsule ? p.ay + pick(-300, 300) : p.ay;
      if (kind == 1 || kind == 2) p.bx = p.ax, p.by = p.ay, p.capsule = 0;
      if (kind == 3) p = DrawPrim{8, 8, 16 * kW - 8, 16 * kH - 8, pick(1, 64), 1, 0, 0u};  // corner to corner: every tile
      p.alpha = pick(0, 256), p.colour = (unsigned)(b * 1000 + i);                       // the colour tells the primitives apart
      const bool in = bins.add(p);
      given[b].push_back(p), kept[b].push_back(in);
      bool any = false;
      for (int y = 0; y < kH && !any; ++y)
        for (int x = 0; x < kW && !any; ++x) any = centre_in_box(p, x, y);
      EXPECT(in == any, "frame %d primitive %d: add() says %d, a pixel centre in its grown box: %d\n", b, i, (int)in, (int)any);
      n_outside += !in, n_everywhere += kind == 3, n_radius1 += p.r16 == 1 && in;
    }
    EXPECT(bins.close_frame(b), "frame %d: close_frame reports more than 2^30 pairs\n", b);
  }
  EXPECT(n_outside > 20 && n_everywhere > 20 && n_radius1 > 5, "the scene lost its cases: %d outside, %d everywhere, %d of radius 1\n", n_outside,
         n_everywhere, n_radius1);

  // wholly-outside primitives are absent from prims; the others are there in the order they were added
  std::vector<int> frame_of;  // of every kept primitive
  size_t at = 0;
  for (int b = 0; b < kFrames; ++b)
    for (size_t i = 0; i < given[b].size(); ++i) {
      if (!kept[b][i]) continue;
      EXPECT(at < bins.prims.size() && same(bins.prims[at], given[b][i]), "prims[%zu] is not frame %d's primitive %zu\n", at, b, i);
      frame_of.push_back(b), ++at;
    }
  EXPECT(at == bins.prims.size(), "prims holds %zu primitives, %zu were kept\n", bins.prims.size(), at);

  // tiles: frame order, then row, then column; none empty; the stretches follow each other and sum to the index length
  size_t next = 0, total = 0;
  std::vector<int> tile_at((size_t)kFrames * kTilesX * kTilesY, -1);
  for (size_t k = 0; k < bins.tiles.size(); ++k) {
    const DrawTile& t = bins.tiles[k];
    EXPECT(t.frame >= 0 && t.frame < kFrames && t.tx >= 0 && t.tx < kTilesX && t.ty >= 0 && t.ty < kTilesY, "tile %zu is (%d, %d, %d)\n", k, t.frame,
           t.tx, t.ty);
    const size_t key = ((size_t)t.frame * kTilesY + t.ty) * kTilesX + t.tx;
    EXPECT(k == 0 || key > next, "tile %zu (%d, %d, %d) is out of order\n", k, t.frame, t.tx, t.ty);
    next = key, tile_at[key] = (int)k;
    EXPECT(t.count > 0, "tile %zu is empty\n", k);
    EXPECT((size_t)t.first == total, "tile %zu starts at %d, the tiles before it hold %zu\n", k, t.first, total);
    total += (size_t)t.count;
    EXPECT(total <= bins.index.size(), "tile %zu ends at %zu, past the index (%zu)\n", k, total, bins.index.size());
    for (int i = 0; i < t.count; ++i) {
      const int id = bins.index[(size_t)t.first + i];
      EXPECT(id >= 0 && (size_t)id < bins.prims.size(), "tile %zu lists primitive %d of %zu\n", k, id, bins.prims.size());
      EXPECT(i == 0 || id > bins.index[(size_t)t.first + i - 1], "tile %zu: its indices do not ascend at %d\n", k, i);
      EXPECT(frame_of[(size_t)id] == t.frame, "tile %zu of frame %d lists primitive %d of frame %d\n", k, t.frame, id, frame_of[(size_t)id]);
    }
  }
  EXPECT(total == bins.index.size(), "the counts sum to %zu, the index holds %zu\n", total, bins.index.size());

  // a tile lists a primitive exactly when it holds a pixel whose centre lies in the primitive's grown box; touched exactly with a tile
  for (int b = 0; b < kFrames; ++b) {
    bool has_tile = false;
    for (int ty = 0; ty < kTilesY; ++ty)
      for (int tx = 0; tx < kTilesX; ++tx) {
        const int k = tile_at[((size_t)b * kTilesY + ty) * kTilesX + tx];
        has_tile = has_tile || k >= 0;
        for (size_t id = 0; id < bins.prims.size(); ++id) {
          if (frame_of[id] != b) continue;
          bool listed = false;
          for (int i = 0; k >= 0 && i < bins.tiles[(size_t)k].count; ++i) listed = listed || bins.index[(size_t)bins.tiles[(size_t)k].first + i] == (int)id;
          const bool want = tile_holds(bins.prims[id], tx, ty);
          EXPECT(listed == want, "frame %d tile (%d, %d) primitive %zu: listed %d, holds a pixel centre of its box %d\n", b, tx, ty, id, (int)listed,
                 (int)want);
        }
      }
    EXPECT((bins.touched[(size_t)b] != 0) == has_tile, "frame %d: touched %d, has a tile %d\n", b, (int)bins.touched[(size_t)b], (int)has_tile);
  }
  EXPECT(!bins.touched[1] && bins.touched[0] && bins.touched[2], "frame 1 gets nothing, frames 0 and 2 do\n");

  // the block the kernels are given: the three arrays at their places
  std::vector<unsigned char> block(bins.bytes(), 0xA5);
  bins.pack(block.data());
  EXPECT(bins.index_at() % 256 == 0 && bins.prims_at() % 256 == 0 && bins.bytes() % 256 == 0, "the parts are not rounded to 256 bytes\n");
  EXPECT(!std::memcmp(block.data(), bins.tiles.data(), bins.tiles.size() * sizeof(DrawTile)) &&
             !std::memcmp(block.data() + bins.index_at(), bins.index.data(), bins.index.size() * sizeof(int)) &&
             !std::memcmp(block.data() + bins.prims_at(), bins.prims.data(), bins.prims.size() * sizeof(DrawPrim)),
         "pack() did not place the arrays\n");
  std::printf("tile_bins_check: %zu primitives kept of %zu, %zu tiles, %zu pairs: OK\n", bins.prims.size(), given[0].size() + given[2].size(),
              bins.tiles.size(), bins.index.size());
  return 0;
}
