// track.hip — people from frame to frame: the association of one frame's people with a slot's live tracks, greedy (step 4) or by
// optimal assignment (step 4'), chosen per tracker (gfx950).
//
// PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker.  The rule is this project's own
// (include/deepcut_hip.h, dc_tracker_update), restated in float64 in tests/track_ref.py.
//
// One latency-class kernel behind assemble_kernel (people.hip) or behind an upload of host poses, nothing of it on the forward path.
// One workgroup per slot walks the images a slot map gives to its slot, so that several frames of one video are tracked in one launch.
// All arithmetic is double and there is no matrix instruction in it: a frame is at most 256 x 256 distances of at most 32 joints.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dc {

namespace {
constexpr int kTrackMax = kPeopleMaxPeople;  // T and P: one thread per track place and per person
constexpr int kTrackBlock = 16;              // track places whose predicted joints sit in LDS at a time (distances)

// the smaller of two (value, index) keys, index ascending among equal values; kNone = no key
constexpr int kNone = 0x7fffffff;
__device__ __forceinline__ void key_min(double& v, int& e, double v2, int e2) {
  if (e2 != kNone && (e == kNone || v2 < v || (v2 == v && e2 < e))) v = v2, e = e2;
}
// ... over the 64 lanes of a wave: every lane ends with the wave's key
__device__ __forceinline__ void wave_key_min(double& v, int& e) {
  for (int s = 32; s > 0; s >>= 1) {
    const double v2 = __shfl_xor(v, s);
    const int e2 = __shfl_xor(e, s);
    key_min(v, e, v2, e2);
  }
}
}  // namespace

// Step 4' (include/deepcut_hip.h): the optimal assignment of the frame's n people to the slot's live tracks by the shortest augmenting
// path Hungarian method, by the whole workgroup, behind a barrier that follows the last store to D.  -> tm[i] / pm[q] of the matched
// pairs; the caller's barrier follows.  The rule is the procedure of the header, scan order included, so this is that procedure and no
// other: per row r an inner loop of at most m + 1 trips, each of which prices the open columns against row i0, takes their arg-min
// (delta, j1) and moves the duals, then one thread walks the augmenting path back.
// Columns go to threads with a stride of 256: thread t owns j = t + 1 and j = t + 257.  People are n <= 256, so the first is a real
// column (person t) when t < n and the second is always a dummy; the row i0 of D is therefore one coalesced read of n doubles, from
// the scratch step 4 reads.  v[j], minv[j] and used[j] are touched by the owner of column j only — they live in its registers, two of
// each; what other threads read is in LDS: u (the owner of a used column moves the dual of ITS row, every thread reads u[i0]), p and
// way (the thread that walks the path reads them all).  (delta, j1) is key_min's (value, index) order: the lowest j among equal
// minima, which is the strict `<` of the ascending scan.  A trip is two barriers, a row one more.  j0 and every exit test derive from LDS values read
// behind a barrier — the four keys, p — so they are the same in every thread.  Both loops carry their bound as a hard trip limit: a
// finite dummy column is always open, so delta is finite and the limits are never reached, but no input may make a workgroup spin.
// Only subtract, add and compare, in the header's order (C - u[i0]) - v[j]; nothing here for the compiler to contract or reassociate.
__device__ __forceinline__ void match_optimal(int T, int P, int n, double max_dist, const double* __restrict__ D, const int* live, int* tm,
                                              int* pm) {
  __shared__ double u[kTrackMax + 1];   // row duals, rows 1..R
  __shared__ int p[2 * kTrackMax + 1];  // the row on column j (0 = none); p[0] = the row being inserted
  __shared__ int way[2 * kTrackMax + 1];
  __shared__ int rowp[kTrackMax];  // the place of row r, at r - 1
  __shared__ double red_v[4];
  __shared__ int red_e[4];
  __shared__ int nrow_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const double inf = __builtin_huge_val();
  if (t < T && live[t]) {
    int rank = 0;
    for (int i = 0; i < t; ++i) rank += live[i];
    rowp[rank] = t;
  }
  if (t == 0) {
    int total = 0;
    for (int i = 0; i < T; ++i) total += live[i];
    nrow_s = total;
  }
  u[t] = 0.0, p[t] = 0, p[t + 256] = 0, way[t] = 0, way[t + 256] = 0;
  if (t == 0) u[256] = 0.0, p[512] = 0, way[512] = 0;
  __syncthreads();
  const int R = nrow_s, m = n + R;
  const int j_a = t + 1, j_b = t + 257;  // this thread's columns
  const bool in_a = j_a <= m, in_b = j_b <= m, real_a = t < n;
  double v_a = 0.0, v_b = 0.0;
  for (int r = 1; r <= R; ++r) {
    double minv_a = inf, minv_b = inf;
    bool used_a = false, used_b = false;
    int j0 = 0;
    if (t == 0) p[0] = r;
    for (int trip = 0; trip <= m; ++trip) {
      __syncthreads();  // the duals of the trip before, p after the walk of the row before, p[0]; red_v / red_e are free again
      if (j0 == j_a) used_a = true;
      if (j0 == j_b) used_b = true;
      const int i0 = p[j0];
      const double ui0 = u[i0];
      double dv = inf;
      int de = kNone;
      if (in_a && !used_a) {
        double c = max_dist;
        if (real_a) {
          const double d = D[(size_t)rowp[i0 - 1] * P + t];
          c = d <= max_dist ? d : inf;
        }
        const double cur = (c - ui0) - v_a;
        if (cur < minv_a) minv_a = cur, way[j_a] = j0;
        if (minv_a < inf) dv = minv_a, de = j_a;
      }
      if (in_b && !used_b) {
        const double cur = (max_dist - ui0) - v_b;
        if (cur < minv_b) minv_b = cur, way[j_b] = j0;
        if (minv_b < inf) key_min(dv, de, minv_b, j_b);
      }
      wave_key_min(dv, de);
      if (lane == 0) red_v[wave] = dv, red_e[wave] = de;
      __syncthreads();
      double delta = red_v[0];
      int j1 = red_e[0];
      for (int w = 1; w < 4; ++w) key_min(delta, j1, red_v[w], red_e[w]);
      if (j1 == kNone) break;  // no open column with a finite price: cannot happen (a dummy is always open); uniform
      if (t == 0) u[r] += delta;  // column 0 is always used and holds row r (v[0] is never read)
      if (in_a) {
        if (used_a) u[p[j_a]] += delta, v_a -= delta;
        else minv_a -= delta;
      }
      if (in_b) {
        if (used_b) u[p[j_b]] += delta, v_b -= delta;
        else minv_b -= delta;
      }
      j0 = j1;
      if (p[j0] == 0) break;  // p does not change inside this loop, j1 came from LDS: uniform
    }
    __syncthreads();  // everybody is done with p (the exit test, the rows of the used columns) before the walk rewrites it
    if (t == 0 && j0 != 0 && p[j0] == 0) {  // way[] of this row is in place: its last stores precede the barriers above
      for (int k = 0; k <= m && j0 != 0; ++k) {
        const int j1 = way[j0];
        p[j0] = p[j1];
        j0 = j1;
      }
    }
  }
  __syncthreads();
  if (t < n) {
    const int r = p[t + 1];
    if (r != 0) {
      const int i = rowp[r - 1];
      pm[t] = i, tm[i] = t;
    }
  }
}

// Step 8 (include/deepcut_hip.h): the smoothed poses of image b and the slot's filters, behind step 7 by the whole workgroup.  The caller
// hands over what steps 4-7 left: live / tm / mult (LDS, as of the start of the update: mult = misses + 1), and per thread q < n the
// place of person q (my_place, -1 = none) and whether the person was born into it.  Items are (person, joint) pairs for 8a / 8c and
// (place, joint) pairs for 8b, strided over the 256 threads; a (place, joint) filter is touched by exactly one item of one of the two
// loops — by the person's item when the place was matched or born, by the place's item otherwise — so no barrier stands between them.
// The filters are read AND written across the images of a launch with the caller's barrier in between: no __restrict__ on them.
__device__ __forceinline__ void smooth_image(int b, int P, int n, const TrackParams& tp, const TrackSmooth& sm, TrackFilter* filt,
                                             const double* __restrict__ ppl, const int* live, const int* tm, const int* mult, int my_place,
                                             bool born) {
  __shared__ int pplace[kTrackMax];   // per person: its place, + kTrackMax when born into it, -1 = untracked
  __shared__ double psize[kTrackMax]; // per person: the step-1 size of its pose
  __shared__ int pkind[kTrackMax];    // per place: 0 = a person's item updates it (8a), 1 = live and unmatched (8b), 2 = free
  const int t = threadIdx.x, T = tp.T, J = tp.J;
  const double inf = __builtin_huge_val();
  constexpr double kTwoPi = 6.283185307179586;
  if (t < n) {
    pplace[t] = my_place < 0 ? -1 : my_place + (born ? kTrackMax : 0);
    double x0 = inf, x1 = -inf, y0 = inf, y1 = -inf;
    for (int j = 0; j < J; ++j) {
      const double* p = ppl + ((size_t)t * J + j) * 3;
      if (p[2] > 0.0) x0 = fmin(x0, p[0]), x1 = fmax(x1, p[0]), y0 = fmin(y0, p[1]), y1 = fmax(y1, p[1]);
    }
    double s = tp.min_size;
    if (x1 >= x0) s = fmax(s, fmax(x1 - x0, y1 - y0));
    psize[t] = s;
  }
  // a place a person was born into is free here (2) and is not touched by the second loop before the person's item has cleared it:
  // the barrier below is followed by the override
  if (t < T) pkind[t] = live[t] ? (tm[t] >= 0 ? 0 : (mult[t] > tp.max_misses ? 2 : 1)) : 2;
  __syncthreads();
  if (t < n && my_place >= 0 && born) pkind[my_place] = 0;
  __syncthreads();

  double* out = sm.smooth + (size_t)b * P * J * 3;
  int* src = sm.src + (size_t)b * P * J;
  const int* cin = sm.cand_in ? sm.cand_in + (size_t)b * P * J : nullptr;
  int* cout = sm.cand_in ? sm.cand_out + (size_t)b * P * J : nullptr;
  for (int e = t; e < P * J; e += 256) {
    const int q = e / J, j = e - q * J;
    double ox = 0.0, oy = 0.0, os = 0.0;
    int sr = 0;
    if (q < n) {
      const double px = ppl[(size_t)e * 3], py = ppl[(size_t)e * 3 + 1], ps = ppl[(size_t)e * 3 + 2];
      const bool held = ps > 0.0;
      const int pl = pplace[q];
      if (pl < 0) {  // 8c
        ox = px, oy = py, os = ps, sr = held ? 1 : 0;
      } else {  // 8a
        TrackFilter* f = filt + (size_t)(pl & (kTrackMax - 1)) * J + j;
        TrackFilter g = *f;
        if (pl >= kTrackMax) g.n = 0;  // born: cleared first
        if (held) {
          if (g.n == 0) {
            g.fx = px, g.fy = py, g.dx = 0.0, g.dy = 0.0, g.n = 1;
            ox = px, oy = py;
          } else if (g.n == 1) {
            const double dt = (double)(g.gap + 1);
            g.dx = (px - g.fx) / dt, g.dy = (py - g.fy) / dt;
            g.fx = px, g.fy = py, g.n = 2;
            ox = px, oy = py;
          } else {
            const double dt = (double)(g.gap + 1);
            const double qx = g.fx + g.dx * dt, qy = g.fy + g.dy * dt;
            const double ex = px - qx, ey = py - qy;
            const double fc = sm.min_cutoff + sm.beta * ((fabs(ex) + fabs(ey)) / psize[q]);
            const double ra = (kTwoPi * fc) * dt, rb = (kTwoPi * sm.d_cutoff) * dt;
            const double a = ra / (ra + 1.0), bb = rb / (rb + 1.0);
            g.fx = qx + a * ex, g.fy = qy + a * ey;
            g.dx = g.dx + bb * (ex / dt), g.dy = g.dy + bb * (ey / dt);
            ox = g.fx, oy = g.fy;
          }
          g.fs = ps, g.gap = 0;
          os = ps, sr = 1;
        } else if (g.n > 0) {
          g.gap += 1;
          if (g.gap > sm.max_hold) {
            g.n = 0;
          } else {
            const double gp = (double)g.gap;
            ox = g.fx + g.dx * gp, oy = g.fy + g.dy * gp, os = g.fs, sr = 2;
          }
        }
        *f = g;
      }
    }
    out[(size_t)e * 3] = ox, out[(size_t)e * 3 + 1] = oy, out[(size_t)e * 3 + 2] = os;
    src[e] = sr;
    if (cin) cout[e] = sr == 2 ? -3 : cin[e];
  }
  for (int e = t; e < T * J; e += 256) {
    const int k = pkind[e / J];
    if (k == 0) continue;
    TrackFilter* f = filt + e;
    if (k == 2) {
      f->n = 0;
    } else if (f->n > 0) {  // 8b
      const int gap = f->gap + 1;
      f->gap = gap;
      if (gap > sm.max_hold) f->n = 0;
    }
  }
}

// ---- the appearance steps 0', 5', 6', 7' (include/deepcut_hip.h, dc_tracker_update_appearance): all integer, so nothing here depends on
// an order of evaluation.  Their LDS lives in one struct behind a function, so that only the instances with Appear hold it.
static_assert(kTrackModel == kAppearDesc, "a model is a quantised descriptor");
struct AppearLds {
  int pvalid[kTrackMax];  // per person: the descriptor is valid (its quantised form is in qdesc)
  int flag[kTrackMax];
  int cand[kTrackMax];    // step 6': the places that enter the gallery, ascending
  int gocc[kTrackGallery];  // the gallery's occupancy as the steps leave it
  int gsrc[kTrackGallery];  // step 6': the place whose model entry g takes, -1 = none
  unsigned key;
  int ncand;
};
__device__ __forceinline__ AppearLds& appear_lds() {
  __shared__ AppearLds lds;
  return lds;
}
// A(m, q) = 12288 - sum min(m, q)
__device__ __forceinline__ int appear_dissim(const int* m, const int* q) {
  int s = 0;
  for (int e = 0; e < kTrackModel; ++e) s += min(m[e], q[e]);
  return 3 * 4096 - s;
}
// m + (((q - m) * alpha256 + 128) >> 8), the shift arithmetic; |q - m| <= 4104, so the product stays below 2^21
__device__ __forceinline__ int appear_blend(int m, int q, int alpha256) { return m + (((q - m) * alpha256 + 128) >> 8); }

// Step 0' and the quantised descriptors of image b, by the whole workgroup in front of step 1 (whose barrier follows): thread e < 64 ages
// gallery entry e and frees it beyond max_age; thread q < n quantises person q's descriptor into qdesc when it is valid.
__device__ __forceinline__ void appear_begin(int b, int P, int n, const TrackAppear& ap, const TrackAppearSlot& as) {
  AppearLds& L = appear_lds();
  const int t = threadIdx.x;
  if (t < kTrackGallery && as.gocc[t]) {
    const int age = as.gage[t] + 1;
    as.gage[t] = age;
    if (age > ap.max_age) as.gocc[t] = 0;
  }
  int ok = 0;
  if (t < n && ap.desc) {
    const int* h = ap.desc + ((size_t)b * P + t) * kTrackModel;
    int* q = ap.qdesc + ((size_t)b * P + t) * kTrackModel;
    long long cnt = 0;
    for (int k = 0; k < kAppearBins; ++k) cnt += h[k];
    if (cnt >= ap.min_pixels && cnt > 0) {
      ok = 1;
      for (int e = 0; e < kTrackModel; ++e) q[e] = (int)((4096LL * h[e] + cnt / 2) / cnt);
    }
  }
  L.pvalid[t] = ok;
}

// Steps 5' and 6' behind steps 5 and 6 (and a barrier), in front of step 7, by the whole workgroup; live / tm / mult as of the start of the
// update.  5': thread i of a matched track whose person has a valid descriptor updates the track's model.  6': the places freed in this
// update with hits >= min_hits and a valid model are listed in ascending order; wave 0 — lane e holds gallery entry e — takes them one by
// one: the lowest free entry (a ballot), else the entry of largest age, the lower index among equals (a wave maximum of age << 6 |
// 63 - e); then the models of the entries that changed hands are copied.  A freed track's id, hits and model are still in place: step 7
// has not run.  The barrier at the end stands between the copies and step 7' 's stores to the models of reborn places.
__device__ __forceinline__ void appear_tracks(int b, int P, const TrackParams& tp, const TrackAppear& ap, const TrackAppearSlot& as,
                                              const TrackSlot& st, const int* live, const int* tm, const int* mult) {
  AppearLds& L = appear_lds();
  const int t = threadIdx.x, T = tp.T;
  int enters = 0;
  if (t < T && live[t]) {
    if (tm[t] >= 0) {
      if (L.pvalid[tm[t]]) {
        const int* q = ap.qdesc + ((size_t)b * P + tm[t]) * kTrackModel;
        int* m = as.model + (size_t)t * kTrackModel;
        const int had = as.valid[t];
        for (int e = 0; e < kTrackModel; ++e) m[e] = had ? appear_blend(m[e], q[e], ap.alpha256) : q[e];
        as.valid[t] = 1;
      }
    } else if (mult[t] > tp.max_misses) {
      enters = (st.hits[t] >= ap.min_hits && as.valid[t]) ? 1 : 0;
    }
  }
  L.flag[t] = enters;
  if (t < kTrackGallery) L.gocc[t] = as.gocc[t], L.gsrc[t] = -1;  // as.gocc[t]: this thread's own store of step 0'
  __syncthreads();
  if (enters) {
    int rank = 0;
    for (int i = 0; i < t; ++i) rank += L.flag[i];
    L.cand[rank] = t;
  }
  if (t == 0) {
    int total = 0;
    for (int i = 0; i < T; ++i) total += L.flag[i];
    L.ncand = total;
  }
  __syncthreads();
  if (t < kTrackGallery) {  // wave 0, all of it
    int occ = L.gocc[t], age = occ ? as.gage[t] : 0, src = -1;
    const int k = L.ncand;
    for (int c = 0; c < k; ++c) {  // k is the same in every lane
      const unsigned long long free_mask = __ballot(!occ);
      int target;
      if (free_mask) {
        target = __ffsll((long long)free_mask) - 1;
      } else {
        int key = (age << 6) | (kTrackGallery - 1 - t);  // age <= 100000 < 2^17
        for (int sft = 32; sft > 0; sft >>= 1) key = max(key, __shfl_xor(key, sft));
        target = kTrackGallery - 1 - (key & (kTrackGallery - 1));
      }
      if (t == target) occ = 1, age = 0, src = L.cand[c];
    }
    L.gocc[t] = occ, L.gsrc[t] = src;
    if (src >= 0) as.gocc[t] = 1, as.gage[t] = 0, as.gid[t] = st.id[src];
  }
  __syncthreads();
  for (int e = t; e < kTrackGallery * kTrackModel; e += 256) {
    const int g = e / kTrackModel, src = L.gsrc[g];
    if (src >= 0) as.gmodel[e] = as.model[(size_t)src * kTrackModel + (e - g * kTrackModel)];
  }
  __syncthreads();
}

// Step 7' in the place of step 7's ids, by the whole workgroup: thread q of a person born into my_place (born) -> the person's id; `got`
// >= 0: re-identified with that gallery entry.  A born person with a valid descriptor keeps its best open entry (smallest A <= reid_max,
// the lower entry among equals); a round takes the smallest key A | entry | person over the workgroup — an LDS atomic minimum, and a
// minimum does not depend on arrival order —, gives the person the entry, frees it, and the people whose best it was look again.  At most
// 64 rounds: every round frees an entry.  The exit test reads LDS behind a barrier: uniform.  Then the ids: the entry's, or next_id + the
// rank among the born people not re-identified; the models of the born places; next_id; the gallery's occupancy back to the state.
__device__ __forceinline__ long long appear_births(int b, int P, int n, const TrackAppear& ap, const TrackAppearSlot& as, const TrackSlot& st,
                                                   bool born, int my_place, long long next_id, int& got) {
  AppearLds& L = appear_lds();
  const int t = threadIdx.x;
  const int* q = ap.qdesc + ((size_t)b * P + t) * kTrackModel;
  const bool want = born && L.pvalid[t];
  int best_a = 0, best_e = -1;
  got = -1;
  auto look = [&]() {
    best_e = -1;
    for (int e = 0; e < kTrackGallery; ++e) {
      if (!L.gocc[e]) continue;
      const int a = appear_dissim(as.gmodel + (size_t)e * kTrackModel, q);
      if (a <= ap.reid_max && (best_e < 0 || a < best_a)) best_a = a, best_e = e;
    }
  };
  if (want) look();
  for (int round = 0; round < kTrackGallery; ++round) {
    if (t == 0) L.key = 0xffffffffu;
    __syncthreads();
    if (want && got < 0 && best_e >= 0) atomicMin(&L.key, ((unsigned)(best_a + 64) << 14) | ((unsigned)best_e << 8) | (unsigned)t);  // A >= -24
    __syncthreads();
    const unsigned key = L.key;
    if (key == 0xffffffffu) break;  // nobody has an entry left: the same value in every thread
    const int we = (int)(key >> 8) & (kTrackGallery - 1), wq = (int)(key & 255u);
    __syncthreads();  // everybody has read the key before it is reset, and gocc before it changes
    if (t == wq) got = we;
    if (t == 0) L.gocc[we] = 0;
    __syncthreads();
    if (want && got < 0 && best_e == we) look();
  }
  __syncthreads();
  L.flag[t] = (born && got < 0) ? 1 : 0;
  __syncthreads();
  long long my_id = -1;
  if (born) {
    int* m = as.model + (size_t)my_place * kTrackModel;
    if (got >= 0) {
      my_id = as.gid[got];
      const int* gm = as.gmodel + (size_t)got * kTrackModel;
      for (int e = 0; e < kTrackModel; ++e) m[e] = appear_blend(gm[e], q[e], ap.alpha256);
      as.valid[my_place] = 1;
    } else {
      int rank = 0;
      for (int i = 0; i < t; ++i) rank += L.flag[i];
      my_id = next_id + rank;
      const int ok = L.pvalid[t];
      if (ok)
        for (int e = 0; e < kTrackModel; ++e) m[e] = q[e];
      as.valid[my_place] = ok;
    }
    st.id[my_place] = my_id;
  }
  if (t == 0) {
    int fresh = 0;
    for (int i = 0; i < n; ++i) fresh += L.flag[i];
    *st.next_id = next_id + fresh;
  }
  if (t < kTrackGallery) as.gocc[t] = L.gocc[t];
  return my_id;
}

// One workgroup of 256 threads (4 waves) applies one image to one slot: the body of an update, steps 1-7.  Thread i owns track place i
// in steps 1, 5 and 6, thread q owns person q in step 7.  D lives in global scratch (256 x 256 doubles do not fit in LDS beside the rest)
// and is written and read inside this workgroup only, with a barrier in between.
// Matching, step 4': match_optimal above.  Step 4: a round takes the smallest D among unmatched pairs.  Scanning all T*P entries every
// round is 256 rounds of 65 536 reads at
// T = P = 256, so the minimum of every ROW is kept in LDS — rv[i], rq[i] = the smallest allowed D of track i among unmatched people and
// the lowest q that has it — and a round is (1) the arg-min over the rows, a (value, place) key whose index order is the tie rule:
// lower place first, and within the row the lower q was kept; (2) the re-derivation of the rows the match invalidates: those whose
// minimum sat at the person just taken.  A wave re-derives a row with coalesced reads and a shuffle reduction; rows go to waves round
// robin.  No step depends on thread timing: same inputs, same ids.
// The state block is read AND written here, and track_kernel calls this several times on one block with a barrier in between: `state`
// carries no __restrict__, so that nothing loaded from it is kept across that barrier.
// Smooth (step 8, TrackSmooth): a second parameter for the same reason — the instances without it are the kernels they were.
// Appear (steps 0', 5', 6', 7', TrackAppear): a third one, likewise: everything of it stands behind `if constexpr (Appear == 1)`.
template <int Assign, int Smooth, int Appear>  // the matching rule, TrackParams::assign: the greedy instance is the kernel it was, instruction for instruction
__device__ __forceinline__ void track_image(int b, unsigned char* state_block, int P, const TrackParams& tp,
                                            const double* __restrict__ sig2_g, double* __restrict__ dist,
                                            const int* __restrict__ n_people, const double* __restrict__ people,
                                            long long* __restrict__ ids, int* __restrict__ place, const TrackSmooth& sm, TrackFilter* filt,
                                            const TrackAppear& ap, unsigned char* appear_block) {
  __shared__ double s2[kTrackMax];   // s_i^2
  __shared__ double rv[kTrackMax];   // row minima: value ...
  __shared__ int rq[kTrackMax];      // ... and person, -1 = the row has no allowed entry left
  __shared__ int live[kTrackMax];    // the place holds a track (as of the start of the update; step 6 clears it)
  __shared__ int mult[kTrackMax];    // misses + 1 of the track
  __shared__ int tm[kTrackMax];      // the person matched to track i, or -1
  __shared__ int pm[kTrackMax];      // the place matched to person q, or -1
  __shared__ int fplace[kTrackMax];  // the free places in ascending order
  __shared__ int flag[kTrackMax];
  __shared__ double sig2[kPeopleMaxJoints];
  __shared__ double bpx[kTrackBlock][kPeopleMaxJoints], bpy[kTrackBlock][kPeopleMaxJoints];  // predicted joints of a block of tracks
  __shared__ int bheld[kTrackBlock][kPeopleMaxJoints];                                        // ... and whether the track holds them
  __shared__ double red_v[4];
  __shared__ int red_e[4];
  __shared__ int nfree_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int T = tp.T, J = tp.J;
  const double inf = __builtin_huge_val();
  const TrackSlot st = track_slot(state_block, T, J);
  const int n = min(max(n_people[b], 0), P);
  const double* ppl = people + (size_t)b * P * J * 3;
  double* D = dist + (size_t)b * T * kTrackMax;
  TrackAppearSlot as{};
  if constexpr (Appear == 1) {
    as = track_appear_slot(appear_block, T);
    appear_begin(b, P, n, ap, as);  // 0'
  }

  // 1. track sizes
  if (t < J) sig2[t] = sig2_g[t];
  tm[t] = -1, pm[t] = -1, rq[t] = -1, rv[t] = inf;
  {
    int lv = 0, ms = 0;
    double size2 = 0.0;
    if (t < T) {
      lv = st.live[t];
      ms = st.misses[t];
      if (lv) {
        double x0 = inf, x1 = -inf, y0 = inf, y1 = -inf;
        for (int j = 0; j < J; ++j) {
          const double* p = st.pose + ((size_t)t * J + j) * 3;
          if (p[2] > 0.0) x0 = fmin(x0, p[0]), x1 = fmax(x1, p[0]), y0 = fmin(y0, p[1]), y1 = fmax(y1, p[1]);
        }
        double s = tp.min_size;
        if (x1 >= x0) s = fmax(s, fmax(x1 - x0, y1 - y0));
        size2 = s * s;
      }
    }
    live[t] = lv, mult[t] = ms + 1, s2[t] = size2;
  }
  __syncthreads();

  // 2., 3. distances, kTrackBlock track places at a time: their predicted joints go to LDS once, then a thread holds one joint of
  // person q in registers and reads tracks of the block from LDS (one address per wave or per P lanes: broadcasts) — a person's pose
  // is fetched T / kTrackBlock times, not T times.  With P < 256 the threads form G = 256 / P slices that share the block's tracks
  // between them.  The sum of a (track, person) pair still runs over the joints ascending, in one thread.
  const int G = min(256 / P, kTrackBlock);
  for (int i0 = 0; i0 < T; i0 += kTrackBlock) {
    __syncthreads();  // the readers of the previous block are done
    for (int e = t; e < kTrackBlock * J; e += 256) {
      const int r = e / J, j = e - r * J, i = i0 + r;
      double px = 0.0, py = 0.0;
      int held = 0;
      if (i < T && live[i]) {
        const double* tr = st.pose + ((size_t)i * J + j) * 3;
        if (tr[2] > 0.0) {
          held = 1, px = tr[0], py = tr[1];
          if (tp.motion == 1) {
            const double* ve = st.vel + ((size_t)i * J + j) * 2;
            const double m = (double)mult[i];
            px = px + ve[0] * m, py = py + ve[1] * m;
          }
        }
      }
      bpx[r][j] = px, bpy[r][j] = py, bheld[r][j] = held;
    }
    __syncthreads();
    if (t < G * P) {  // thread (slice, q): the block's tracks slice, slice + G, ... against person q
      const int slice = t / P, q = t - slice * P;
      double sum[kTrackBlock];
      int nc[kTrackBlock];
#pragma unroll
      for (int k = 0; k < kTrackBlock; ++k) sum[k] = 0.0, nc[k] = 0;
      if (q < n)
        for (int j = 0; j < J; ++j) {
          const double* pe = ppl + ((size_t)q * J + j) * 3;
          const double qx = pe[0], qy = pe[1];
          if (!(pe[2] > 0.0)) continue;
          const double sg = sig2[j];
#pragma unroll
          for (int k = 0; k < kTrackBlock; ++k) {
            const int r = slice + k * G;
            if (r < kTrackBlock && bheld[r][j]) {
              const double dx = bpx[r][j] - qx, dy = bpy[r][j] - qy;
              sum[k] += (dx * dx + dy * dy) / (s2[i0 + r] * sg);
              ++nc[k];
            }
          }
        }
#pragma unroll
      for (int k = 0; k < kTrackBlock; ++k) {
        const int r = slice + k * G;
        if (r < kTrackBlock && i0 + r < T)
          D[(size_t)(i0 + r) * P + q] = (nc[k] >= tp.min_common && nc[k] > 0) ? sum[k] / (double)nc[k] : inf;
      }
    }
  }
  __syncthreads();  // D is complete (global memory written and read by this workgroup only)

  if constexpr (Assign == 1) {
    // 4'. optimal assignment
    match_optimal(T, P, n, tp.max_dist, D, live, tm, pm);
  } else {
    // 4. greedy matching on row minima
    auto row_min = [&](int i) {  // by one wave: rv[i], rq[i] over the unmatched people
      double v = inf;
      int e = kNone;
      for (int q = lane; q < n; q += 64) {
        if (pm[q] >= 0) continue;
        const double d = D[(size_t)i * P + q];
        if (d <= tp.max_dist && d < v) v = d, e = q;  // q ascends within a lane: the first of equal distances stays
      }
      wave_key_min(v, e);
      if (lane == 0) rv[i] = v, rq[i] = e == kNone ? -1 : e;
    };
    for (int i = wave; i < T; i += 4)
      if (live[i]) row_min(i);
    for (;;) {
      __syncthreads();  // the row minima of this round are in place
      double v = inf;
      int e = kNone;
      if (t < T && live[t] && tm[t] < 0 && rq[t] >= 0) v = rv[t], e = t;
      wave_key_min(v, e);
      if (lane == 0) red_v[wave] = v, red_e[wave] = e;
      __syncthreads();
      v = red_v[0], e = red_e[0];
      for (int w = 1; w < 4; ++w) key_min(v, e, red_v[w], red_e[w]);
      if (e == kNone) break;  // the same value in every thread: the exit is uniform
      const int wi = e, wq = rq[wi];
      __syncthreads();  // everybody has read the winner's row before it changes
      if (t == 0) tm[wi] = wq, pm[wq] = wi;
      __syncthreads();
      for (int i = wave; i < T; i += 4)
        if (live[i] && tm[i] < 0 && rq[i] == wq) row_min(i);
    }
  }
  __syncthreads();

  // 5., 6. the tracks
  {
    int free_now = 0;
    if (t < T) {
      if (live[t] && tm[t] >= 0) {
        const double m = (double)mult[t];
        const double* pe = ppl + (size_t)tm[t] * J * 3;
        for (int j = 0; j < J; ++j) {
          double* tr = st.pose + ((size_t)t * J + j) * 3;
          double* ve = st.vel + ((size_t)t * J + j) * 2;
          const double x = pe[j * 3], y = pe[j * 3 + 1], sc = pe[j * 3 + 2];
          double vx = 0.0, vy = 0.0;
          if (tr[2] > 0.0 && sc > 0.0) vx = (x - tr[0]) / m, vy = (y - tr[1]) / m;
          ve[0] = vx, ve[1] = vy;
          tr[0] = x, tr[1] = y, tr[2] = sc;
        }
        st.misses[t] = 0;
        st.hits[t] += 1;
      } else if (live[t]) {
        const int ms = mult[t];  // misses + 1
        st.misses[t] = ms;
        if (ms > tp.max_misses) st.live[t] = 0, free_now = 1;
      } else {
        free_now = 1;
      }
    }
    flag[t] = free_now;
  }
  __syncthreads();
  if constexpr (Appear == 1) appear_tracks(b, P, tp, ap, as, st, live, tm, mult);  // 5', 6'
  // 7. births: the r-th unmatched person takes the r-th free place
  if (flag[t]) {
    int rank = 0;
    for (int i = 0; i < t; ++i) rank += flag[i];
    fplace[rank] = t;
  }
  if (t == 0) {
    int total = 0;
    for (int i = 0; i < T; ++i) total += flag[i];
    nfree_s = total;
  }
  __syncthreads();
  const int unmatched = (t < n && pm[t] < 0) ? 1 : 0;
  const int nfree = nfree_s;
  const long long next_id = *st.next_id;  // read by everybody before thread 0 moves it on, below the next barrier
  __syncthreads();                        // flag is free again
  flag[t] = unmatched;
  __syncthreads();
  long long my_id = -1;
  int my_place = -1;
  if (t < n) {
    if (!unmatched) {
      my_place = pm[t];
      my_id = st.id[my_place];
    } else {
      int rank = 0;
      for (int q = 0; q < t; ++q) rank += flag[q];
      if (rank < nfree) {
        my_place = fplace[rank];
        if constexpr (Appear == 0) my_id = next_id + rank;  // with Appear: step 7', below
        const double* pe = ppl + (size_t)t * J * 3;
        for (int j = 0; j < J; ++j) {
          double* tr = st.pose + ((size_t)my_place * J + j) * 3;
          double* ve = st.vel + ((size_t)my_place * J + j) * 2;
          tr[0] = pe[j * 3], tr[1] = pe[j * 3 + 1], tr[2] = pe[j * 3 + 2];
          ve[0] = 0.0, ve[1] = 0.0;
        }
        if constexpr (Appear == 0) st.id[my_place] = my_id;
        st.live[my_place] = 1;
        st.misses[my_place] = 0;
        st.hits[my_place] = 1;
      }
    }
  }
  if constexpr (Appear == 0) {
    if (t == 0) {
      int born = 0;
      for (int q = 0; q < n; ++q) born += flag[q];
      *st.next_id = next_id + min(born, nfree);
    }
  } else {  // 7': the ids of the born people, from the gallery or from next_id
    const bool born = unmatched && my_place >= 0;
    int got;
    const long long born_id = appear_births(b, P, n, ap, as, st, born, my_place, next_id, got);
    if (born) my_id = born_id;
    if (t < P) ap.reid[(size_t)b * P + t] = got >= 0 ? 1 : 0;
  }
  if (t < P) {
    ids[(size_t)b * P + t] = my_id;
    place[(size_t)b * P + t] = my_place;
  }
  if constexpr (Smooth == 1) smooth_image(b, P, n, tp, sm, filt, ppl, live, tm, mult, my_place, unmatched != 0);
}

// One workgroup per slot: it walks the images in ascending b and applies those the map gives to its slot, each on the state the one
// before left.  The map is a kernel argument and blockIdx is uniform, so the branch is.  The barrier behind an image stands between its
// last stores to the state (steps 5-7) and the next image's loads of it (steps 1-3) by other threads of this workgroup, and between its
// last readers of the LDS arrays (flag, fplace, pm in step 7) and the next image's initialisation of them.  A workgroup whose slot no
// image names returns without touching the slot.
// With Smooth the same barrier stands between an image's stores to the slot's filters (step 8) and the next image's loads of them, with
// Appear between its stores to the slot's models and gallery and the next image's loads of those.
template <int Assign, int Smooth, int Appear>
__global__ __launch_bounds__(256) void track_kernel(int NB, int P, TrackParams tp, TrackSlotMap map, const double* __restrict__ sig2_g,
                                                    unsigned char* state, size_t slot_stride, double* __restrict__ dist,
                                                    const int* __restrict__ n_people, const double* __restrict__ people,
                                                    long long* __restrict__ ids, int* __restrict__ place, TrackSmooth sm, TrackAppear ap) {
  const int slot = blockIdx.x;
  unsigned char* block = state + (size_t)slot * slot_stride;
  TrackFilter* filt = Smooth == 1 ? sm.filt + (size_t)slot * tp.T * tp.J : nullptr;
  unsigned char* appear_block = Appear == 1 ? ap.state + (size_t)slot * ap.slot_stride : nullptr;
  for (int b = 0; b < NB; ++b) {
    if ((int)((map.w[b >> 2] >> ((b & 3) * 8)) & 0xffu) != slot) continue;  // uniform
    track_image<Assign, Smooth, Appear>(b, block, P, tp, sig2_g, dist, n_people, people, ids, place, sm, filt, ap, appear_block);
    __syncthreads();
  }
}

int launch_track(int S, int NB, int P, const TrackParams& p, const double* sig2, unsigned char* state, size_t slot_stride, double* dist,
                 const int* n_people, const double* people, long long* ids, int* place, const TrackSlotMap& map, void* stream,
                 const TrackSmooth* sm, const TrackAppear* ap) {
  if (NB <= 0) return 0;
  if (S < 1 || S > 256 || NB > kTrackMaxImages || P < 1 || P > kTrackMax || p.T < 1 || p.T > kTrackMax || p.J < 1 ||
      p.J > kPeopleMaxJoints || slot_stride % 16 || slot_stride < track_slot_bytes(p.T, p.J) || p.assign < 0 || p.assign > 1)
    return (int)hipErrorInvalidValue;
  for (int b = 0; b < NB; ++b)
    if ((int)((map.w[b >> 2] >> ((b & 3) * 8)) & 0xffu) >= S) return (int)hipErrorInvalidValue;
  if (sm && (!sm->filt || !sm->smooth || !sm->src || (sm->cand_in && !sm->cand_out) || sm->max_hold < 0)) return (int)hipErrorInvalidValue;
  if (ap && (!ap->state || !ap->qdesc || !ap->reid || ap->slot_stride % 8 || ap->slot_stride < track_appear_bytes(p.T) || ap->min_pixels < 1 ||
             ap->alpha256 < 0 || ap->alpha256 > 256 || ap->reid_max < 0 || ap->reid_max > 3 * 4096 || ap->max_age < 0 || ap->max_age > 100000 ||
             ap->min_hits < 1))
    return (int)hipErrorInvalidValue;
  const TrackSmooth off{};
  const TrackAppear plain{};
  auto go = [&](auto kernel, const TrackSmooth& s8, const TrackAppear& a) {
    hipLaunchKernelGGL(kernel, dim3(S), dim3(256), 0, (hipStream_t)stream, NB, P, p, map, sig2, state, slot_stride, dist, n_people, people,
                       ids, place, s8, a);
  };
  // step 4', step 8 and the appearance steps: instantiations of their own, so that the greedy one without either keeps its registers and
  // its LDS
  if (ap) {
    if (sm) p.assign == 1 ? go(track_kernel<1, 1, 1>, *sm, *ap) : go(track_kernel<0, 1, 1>, *sm, *ap);
    else p.assign == 1 ? go(track_kernel<1, 0, 1>, off, *ap) : go(track_kernel<0, 0, 1>, off, *ap);
  } else {
    if (sm) p.assign == 1 ? go(track_kernel<1, 1, 0>, *sm, plain) : go(track_kernel<0, 1, 0>, *sm, plain);
    else p.assign == 1 ? go(track_kernel<1, 0, 0>, off, plain) : go(track_kernel<0, 0, 0>, off, plain);
  }
  return (int)hipGetLastError();
}

}  // namespace dc
