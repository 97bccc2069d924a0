// people.hip — bottom-up assembly of people from the part candidates and the pairwise maps of one forward (gfx950).
//
// PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn has no consumer of `next_pred` (it stops at the maps).  The
// pair cost inverts the label encoding of its training layer (src/caffe/layers/pose_data_layer.cpp:686-802) exactly as
// pairwise_decode_kernel does; the greedy grouping rule is this project's own.
//
// Two latency-class kernels behind part_select_kernel (pose.hip), nothing of them on the forward path:
//   pair_cost_kernel  one workgroup per (image, joint a): cost[b][a][c][i][k] for every partner joint c and candidate pair
//   assemble_kernel   one workgroup per image: the greedy linking, joint after joint, on that cost tensor
// and, only when the caller enabled completion (dc_net_set_completion), a third behind them:
//   complete_kernel   one workgroup per (image, joint j): the joints j that people lack, looked for in the score map around the mean
//                     of the positions their held joints predict (stage D; like B and C this project's own rule)
// and, only when the caller enabled duplicate suppression (dc_net_set_dedupe), or through dc_dedupe_people, one more:
//   dedupe_kernel     one workgroup per image: people ranked by score, everybody a better kept person is "the same" as by the
//                     tracker's distance suppressed, optionally absorbed, the rest compacted (stage E; this project's own rule too)
// All arithmetic is double, like the two decoders.  Double rate does not matter here: a full cost tensor (14 x 14 x 64 x 64) is
// 1.6 M square roots, and the usual one (16 candidates) a sixteenth of it.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dc {

namespace {
template <typename F>
int people_by_kind(int ekind, F&& f) {
  if (ekind == kElemF16) return f((_Float16*)nullptr);
  if (ekind == kElemBF16) return f((__bf16*)nullptr);
  return f((float*)nullptr);
}
}  // namespace

// where regression edge l, read at cell (row, col) of image b, puts the next joint (image pixels): pairwise_decode_kernel's arithmetic
template <typename T>
__device__ __forceinline__ void pair_predict(const T* __restrict__ next, int ncp, int nc0, int b, int H, int W, int row, int col, int l,
                                             const double* __restrict__ mean, const double* __restrict__ stdev, double scale, double& x,
                                             double& y) {
  const T* p = next + (((long)b * H + row) * W + col) * ncp + nc0 + 2 * l;
  x = ((double)col * 8.0 + 4.0 + (double)(float)p[0] * stdev[2 * l] + mean[2 * l]) / scale;
  y = ((double)row * 8.0 + 4.0 + (double)(float)p[1] * stdev[2 * l + 1] + mean[2 * l + 1]) / scale;
}

// Workgroup (b, a) owns the unordered pairs {a, c} with c > a (and the diagonal block, which is +inf): the number is computed once
// and stored at [a][c][i][k] and [c][a][k][i], so every element of the tensor is written exactly once and no atomics are needed.
// LDS (doubles, structure of arrays so that 32 consecutive k are 32 consecutive 8-byte words = every bank once; the i side of a
// read is one address per MD consecutive lanes, a broadcast):
//   fx, fy [J][MD]  prediction of candidate (a, i) towards joint c (edge a -> c), loaded ONCE for every partner
//   ax, ay [MD]     position of candidate (a, i)
//   rx, ry [MD]     per partner: prediction of candidate (c, k) towards joint a (edge c -> a)
//   cx, cy [MD]     per partner: position of candidate (c, k)
// lut[a*J + c] = the lowest edge index l with edges[l] == (a, c), or -1.
template <typename T>
__global__ __launch_bounds__(256) void pair_cost_kernel(const T* __restrict__ next, int ncp, int nc0, int H, int W, int J, int MD,
                                                        double scale, const int* __restrict__ counts, const double* __restrict__ dets,
                                                        const int* __restrict__ lut, const double* __restrict__ mean,
                                                        const double* __restrict__ stdev, double* __restrict__ cost) {
  extern __shared__ double pc_lds[];
  double* fx = pc_lds;
  double* fy = fx + J * MD;
  double* ax = fy + J * MD;
  double* ay = ax + MD;
  double* rx = ay + MD;
  double* ry = rx + MD;
  double* cx = ry + MD;
  double* cy = cx + MD;
  const int ba = blockIdx.x, b = ba / J, a = ba - b * J, t = threadIdx.x;
  const int ma = min(counts[ba], MD);
  const double* da = dets + (long)ba * MD * 5;
  const double inf = __builtin_huge_val();
  auto cell_ok = [&](int row, int col) { return row >= 0 && row < H && col >= 0 && col < W; };
  for (int e = t; e < J * MD; e += 256) {
    const int c = e / MD, i = e - c * MD;
    const int l = lut[a * J + c];
    double x = 0.0, y = 0.0;
    if (i < ma && l >= 0) {
      const int row = (int)da[i * 5 + 3], col = (int)da[i * 5 + 4];
      if (cell_ok(row, col)) pair_predict(next, ncp, nc0, b, H, W, row, col, l, mean, stdev, scale, x, y);
    }
    fx[e] = x, fy[e] = y;
  }
  for (int i = t; i < MD; i += 256) {
    ax[i] = i < ma ? da[i * 5] : 0.0;
    ay[i] = i < ma ? da[i * 5 + 1] : 0.0;
  }
  const long blk = (long)MD * MD;
  double* cb = cost + (long)b * J * J * blk;
  for (int idx = t; idx < MD * MD; idx += 256) cb[((long)a * J + a) * blk + idx] = inf;
  for (int c = a + 1; c < J; ++c) {
    const int mc = min(counts[b * J + c], MD), lf = lut[a * J + c], lr = lut[c * J + a];
    const double* dcand = dets + ((long)b * J + c) * MD * 5;
    __syncthreads();  // the first time: fx .. ay are complete; later: the previous partner's readers are done with rx .. cy
    for (int k = t; k < MD; k += 256) {
      double x = 0.0, y = 0.0, px = 0.0, py = 0.0;
      if (k < mc) {
        px = dcand[k * 5], py = dcand[k * 5 + 1];
        const int row = (int)dcand[k * 5 + 3], col = (int)dcand[k * 5 + 4];
        if (lr >= 0 && cell_ok(row, col)) pair_predict(next, ncp, nc0, b, H, W, row, col, lr, mean, stdev, scale, x, y);
      }
      rx[k] = x, ry[k] = y, cx[k] = px, cy[k] = py;
    }
    __syncthreads();
    double* ac = cb + ((long)a * J + c) * blk;
    double* ca = cb + ((long)c * J + a) * blk;
    for (int idx = t; idx < MD * MD; idx += 256) {
      const int i = idx / MD, k = idx - i * MD;
      double v = inf;
      if (i < ma && k < mc && (lf >= 0 || lr >= 0)) {
        double s = 0.0;
        int n = 0;
        if (lf >= 0) {
          const double dx = fx[c * MD + i] - cx[k], dy = fy[c * MD + i] - cy[k];
          s += sqrt(dx * dx + dy * dy);
          ++n;
        }
        if (lr >= 0) {
          const double dx = rx[k] - ax[i], dy = ry[k] - ay[i];
          s += sqrt(dx * dx + dy * dy);
          ++n;
        }
        v = scale * (s / (double)n);
      }
      ac[(long)i * MD + k] = v;
      ca[(long)k * MD + i] = v;
    }
  }
}

// Greedy assembly of one image by one workgroup.  State in LDS: asg[p][a] = the candidate of joint a that person p holds, or -1.
// Per joint j (in `order`): every (person, candidate) link cost L goes to this image's rows of `link` (global scratch: 256 people x
// 64 candidates of doubles do not fit beside the rest; entry e = p*m + i is written and read by the same thread only), then the
// links are taken one at a time by a workgroup-wide arg-min over (L, e) keys in LDS — e ascending IS (p, i) ascending, the tie rule —
// and the candidates left over seed new people by a prefix count.  No step depends on thread timing: same inputs, same people.
__global__ __launch_bounds__(256) void assemble_kernel(int J, int MD, int P, int min_joints, double max_cost, double seed_thr,
                                                       const int* __restrict__ counts, const double* __restrict__ dets,
                                                       const double* __restrict__ cost, const int* __restrict__ order,
                                                       double* __restrict__ link, int* __restrict__ n_people,
                                                       double* __restrict__ people, int* __restrict__ cand) {
  extern __shared__ int asg[];  // [P][J]
  __shared__ double red_l[256];
  __shared__ int red_e[256];
  __shared__ int flag[256];
  __shared__ int slot[256];
  __shared__ int used[64];
  __shared__ int np_s;
  const int b = blockIdx.x, t = threadIdx.x;
  const double inf = __builtin_huge_val();
  const int kNone = 0x7fffffff;
  const long blk = (long)MD * MD;
  const double* cb = cost + (long)b * J * J * blk;
  double* L = link + (long)b * P * MD;
  for (int e = t; e < P * J; e += 256) asg[e] = -1;
  if (t == 0) np_s = 0;
  __syncthreads();
  for (int oj = 0; oj < J; ++oj) {
    const int j = order[oj];
    const int m = min(counts[b * J + j], MD);
    const int np = np_s;
    const int links = np * m;
    if (t < 64) used[t] = 0;
    // 1. link costs: the mean of the finite pair costs between candidate i and the joints the person already holds, a ascending
    for (int e = t; e < links; e += 256) {
      const int p = e / m, i = e - p * m;
      double s = 0.0;
      int n = 0;
      for (int a = 0; a < J; ++a) {
        const int ia = asg[p * J + a];
        if (a == j || ia < 0) continue;
        const double v = cb[((long)a * J + j) * blk + (long)ia * MD + i];
        if (v < inf && v > -inf) s += v, ++n;
      }
      L[e] = n ? s / (double)n : inf;
    }
    __syncthreads();
    // 2. linking: the smallest allowed link between a person without joint j and a free candidate, until none is left
    for (;;) {
      double bl = inf;
      int be = kNone;
      for (int e = t; e < links; e += 256) {
        const int p = e / m, i = e - p * m;
        if (used[i] || asg[p * J + j] >= 0) continue;
        const double v = L[e];
        if (v <= max_cost && v < bl) bl = v, be = e;  // e ascends within a thread: the first of equal costs stays
      }
      red_l[t] = bl, red_e[t] = be;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
          const double l2 = red_l[t + s];
          const int e2 = red_e[t + s];
          if (e2 != kNone && (red_e[t] == kNone || l2 < red_l[t] || (l2 == red_l[t] && e2 < red_e[t]))) red_l[t] = l2, red_e[t] = e2;
        }
        __syncthreads();
      }
      const int win = red_e[0];  // the same value in every thread: the exit is uniform
      if (win == kNone) break;
      __syncthreads();  // everybody has read the winner before thread 0 of the next round overwrites it
      if (t == 0) {
        const int p = win / m, i = win - p * m;
        asg[p * J + j] = i;
        used[i] = 1;
      }
      __syncthreads();
    }
    // 3. seeding: the free candidates at or above the seed threshold, in list order, while there is room
    __syncthreads();
    if (t < 64) flag[t] = (t < m && !used[t] && dets[(((long)b * J + j) * MD + t) * 5 + 2] >= seed_thr) ? 1 : 0;
    __syncthreads();
    if (t < m && flag[t]) {
      int rank = 0;
      for (int i = 0; i < t; ++i) rank += flag[i];
      if (np + rank < P) asg[(np + rank) * J + j] = t;
    }
    if (t == 0) {
      int total = 0;
      for (int i = 0; i < m; ++i) total += flag[i];
      np_s = min(P, np + total);
    }
    __syncthreads();
  }
  // people with fewer than min_joints joints leave, the others keep their order
  const int np = np_s;
  {
    int nj = 0;
    if (t < np)
      for (int a = 0; a < J; ++a) nj += asg[t * J + a] >= 0;
    flag[t] = (t < np && nj >= min_joints) ? 1 : 0;
  }
  __syncthreads();
  if (flag[t]) {
    int rank = 0;
    for (int i = 0; i < t; ++i) rank += flag[i];
    slot[rank] = t;
  }
  if (t == 0) {
    int total = 0;
    for (int i = 0; i < np; ++i) total += flag[i];
    np_s = total;
    n_people[b] = total;
  }
  __syncthreads();
  const int kept = np_s;
  for (int e = t; e < P * J; e += 256) {
    const int q = e / J, a = e - q * J;
    int ci = -1;
    double x = 0.0, y = 0.0, s = 0.0;
    if (q < kept) {
      ci = asg[slot[q] * J + a];
      if (ci >= 0) {
        const double* d = dets + (((long)b * J + a) * MD + ci) * 5;
        x = d[0], y = d[1], s = d[2];
      }
    }
    double* o = people + ((long)b * P * J + e) * 3;
    o[0] = x, o[1] = y, o[2] = s;
    cand[(long)b * P * J + e] = ci;
  }
}

// Stage D, the completion pass (opt-in; the rule: include/deepcut_hip.h, dc_complete_params).  One workgroup per (image, joint j):
// the cells of the candidates of j that people hold go to LDS first, indexed by the candidate (a candidate is held by at most one
// person, so slot ci is written by one thread and no counter is needed; a free slot stays far off the map), then the four waves walk
// the people of the image, one (person, joint) item per wave.  Lane a computes predictor a (J <= 32 lanes busy); the sum runs over a
// ascending through lane broadcasts, so every lane holds the same e; the lanes then stride over the window — its cells ascend with
// the lane's trips, so the first of equal scores stays within a lane — and an xor-butterfly arg-max over (score, cell) leaves the
// winner in every lane; lane 0 writes.  No atomics, and nothing read here is written here: `cand_in` is stage C's, `cand_out` a
// column of its own per workgroup, and people[b][.][j] is touched by this workgroup alone — the result does not depend on timing.
template <typename T, typename TN>
__global__ __launch_bounds__(256) void complete_kernel(const T* __restrict__ prob, int pcp, int pc0, const T* __restrict__ loc, int lcp,
                                                       int lc0, const TN* __restrict__ next, int ncp, int nc0, int H, int W, int J, int MD,
                                                       int P, double scale, int radius, float fill_thr, int fill_radius, int min_support,
                                                       const double* __restrict__ dets, const int* __restrict__ lut,
                                                       const double* __restrict__ mean, const double* __restrict__ stdev,
                                                       const int* __restrict__ n_people, const int* __restrict__ cand_in,
                                                       double* __restrict__ people, int* __restrict__ cand_out) {
  __shared__ int ex_row[kPeopleMaxDet], ex_col[kPeopleMaxDet];
  const int bj = blockIdx.x, b = bj / J, j = bj - b * J, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = min(max(n_people[b], 0), P);
  const int kFar = -(1 << 20);  // further than any radius from every cell
  const int kNone = 0x7fffffff;
  const int* cin = cand_in + (long)b * P * J;
  const double* dj = dets + (long)bj * MD * 5;
  if (t < kPeopleMaxDet) ex_row[t] = kFar, ex_col[t] = kFar;
  __syncthreads();
  for (int q = t; q < n; q += 256) {
    const int ci = cin[q * J + j];
    if (ci >= 0 && ci < MD) ex_row[ci] = (int)dj[ci * 5 + 3], ex_col[ci] = (int)dj[ci * 5 + 4];
  }
  __syncthreads();
  const T* pj = prob + ((long)b * H * W) * pcp + pc0 + j;
  for (int q = wave; q < P; q += 4) {  // uniform per wave
    const int mine = cin[q * J + j];
    int* co = cand_out + ((long)b * P + q) * J + j;
    if (q >= n || mine >= 0) {
      if (lane == 0) *co = mine;
      continue;
    }
    // 1. predictors: lane a holds pred_a when q holds joint a and an edge a -> j exists
    double px = 0.0, py = 0.0;
    bool have = false;
    if (lane < J && lane != j) {
      const int ia = cin[q * J + lane], l = lut[lane * J + j];
      if (ia >= 0 && ia < MD && l >= 0) {
        const double* da = dets + (((long)b * J + lane) * MD + ia) * 5;
        const int row = (int)da[3], col = (int)da[4];
        if (row >= 0 && row < H && col >= 0 && col < W) {
          pair_predict(next, ncp, nc0, b, H, W, row, col, l, mean, stdev, scale, px, py);
          have = true;
        }
      }
    }
    const unsigned long long who = __ballot(have);
    const int support = __popcll(who);
    // 2. the expected position: the sum over a ascending, the same in every lane
    double sx = 0.0, sy = 0.0;
    for (int a = 0; a < J; ++a) {
      const double ax = __shfl(px, a), ay = __shfl(py, a);
      if ((who >> a) & 1ull) sx += ax, sy += ay;
    }
    float bv = 0.f;
    int bc = kNone;
    if (support >= min_support && support > 0) {
      const double ex = sx / (double)support, ey = sy / (double)support;
      if (ex - ex == 0.0 && ey - ey == 0.0) {  // finite
        // 3. the window, clipped in double: e may lie anywhere
        const double fc = floor(ex * scale / 8.0), fr = floor(ey * scale / 8.0);
        const double c_lo = fmax(fc - (double)fill_radius, 0.0), c_hi = fmin(fc + (double)fill_radius, (double)(W - 1));
        const double r_lo = fmax(fr - (double)fill_radius, 0.0), r_hi = fmin(fr + (double)fill_radius, (double)(H - 1));
        if (c_lo <= c_hi && r_lo <= r_hi) {
          const int c0 = (int)c_lo, r0 = (int)r_lo, ww = (int)c_hi - c0 + 1, wh = (int)r_hi - r0 + 1;
          for (int idx = lane; idx < ww * wh; idx += 64) {
            const int dr = idx / ww, row = r0 + dr, col = c0 + (idx - dr * ww), cell = row * W + col;
            // 4. somebody's peak: within `radius` of a held candidate of j
            bool taken = false;
            for (int k = 0; k < MD; ++k) taken = taken || (abs(row - ex_row[k]) <= radius && abs(col - ex_col[k]) <= radius);
            const float v = (float)pj[(long)cell * pcp];
            // 5. v >= fill_thr is false for a NaN; cells ascend within a lane, so `>` keeps the first of equal scores
            if (!taken && v >= fill_thr && (bc == kNone || v > bv)) bv = v, bc = cell;
          }
        }
      }
    }
    for (int s = 32; s > 0; s >>= 1) {
      const float v2 = __shfl_xor(bv, s);
      const int c2 = __shfl_xor(bc, s);
      if (c2 != kNone && (bc == kNone || v2 > bv || (v2 == bv && c2 < bc))) bv = v2, bc = c2;
    }
    if (lane == 0) {
      if (bc != kNone) {
        const double kLoc = 7.280109889280518;  // sqrt(53), as part_select_kernel
        const int row = bc / W, col = bc - row * W;
        const T* l = loc + (((long)b * H + row) * W + col) * lcp + lc0 + 2 * j;
        double* o = people + (((long)b * P + q) * J + j) * 3;
        o[0] = ((double)col * 8.0 + 4.0 + (double)(float)l[0] * kLoc) / scale;
        o[1] = ((double)row * 8.0 + 4.0 + (double)(float)l[1] * kLoc) / scale;
        o[2] = (double)bv;
        *co = -2;
      } else {
        *co = -1;
      }
    }
  }
}

// Stage E, duplicate suppression (opt-in; the rule: include/deepcut_hip.h, dc_dedupe_params).  One workgroup per image, thread q =
// person q of the input:
//   1. thread q: S_q, s_q^2 and the held mask, joints ascending;
//   2. rank_q = the number of people that rank before q, counted over S in LDS (S is never a NaN: only scores > 0 are summed).  A count
//      needs no 72-bit (S, q) sort key and no order of its own; the poses then go to LDS IN RANK ORDER as a structure of arrays
//      px, py [j][rank]: the 64 lanes of a wave below read 64 consecutive 8-byte words of one joint — each 32-lane half covers the 64
//      banks once — and the better-ranked side of a pair is one address per wave, a broadcast;
//   3. the similarity matrix as bits: a wave takes (rank ra, word w), lane l the pair (ra, rb = 64 w + l) with rb > ra, the sum of a
//      pair runs over the joints ascending in that one lane, and the ballot of the decisions is word w of row ra — every word has one
//      writer;
//   4. wave 0 sweeps the ranks: lane w owns word w of the `removed` set; a kept ra ors its row in and the bits that are new record ra as
//      their killer.  The loop has n trips, whatever the data;
//   5. thread q again: kept people are counted by a prefix over q (ballots and four wave totals), so they keep their input order; then
//      every (output person, joint) item copies its joint, from the first-ranked donor when absorbing.
// Values are copied, never computed: only the decisions depend on arithmetic.  No atomics; the inputs are read only and the outputs
// are buffers of their own, so nothing read here is written here.
struct DedupeSigma {
  double s2[kPeopleMaxJoints];  // sigma_j^2, 1.0 where the caller gave none
};
__global__ __launch_bounds__(256) void dedupe_kernel(int J, int P, double max_dist, int min_common, double min_size, int absorb,
                                                     DedupeSigma sig, const int* __restrict__ n_in, const double* __restrict__ ppl_in,
                                                     const int* __restrict__ cand_in, int* __restrict__ n_out,
                                                     double* __restrict__ ppl_out, int* __restrict__ cand_out,
                                                     int* __restrict__ kept_from, int* __restrict__ supp_by) {
  extern __shared__ double dd_lds[];  // px [J][P], py [J][P], rank order
  __shared__ unsigned long long sim[kPeopleMaxPeople * 4];  // row ra, word w: bit l = rank 64 w + l is similar to ra (and ranks behind it)
  __shared__ double S_s[kPeopleMaxPeople];                  // by person
  __shared__ double s2_s[kPeopleMaxPeople];                 // by rank: s^2
  __shared__ double sig2[kPeopleMaxJoints];
  __shared__ unsigned hm_s[kPeopleMaxPeople];  // by rank: bit j = joint j is held
  __shared__ int order_s[kPeopleMaxPeople];    // rank -> person
  __shared__ int rank_s[kPeopleMaxPeople];     // person -> rank
  __shared__ int by_s[kPeopleMaxPeople];       // by rank: the rank of the kept person that suppressed it, or -1 = kept
  __shared__ int from_s[kPeopleMaxPeople];     // output person -> input person
  __shared__ int wtot[4];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = min(max(n_in[b], 0), P);
  const double inf = __builtin_huge_val();
  const double* pin = ppl_in + (long)b * P * J * 3;
  const int* cin = cand_in + (long)b * P * J;
  double* px = dd_lds;
  double* py = px + J * P;

  // 1. score, size, held
  double S = 0.0, size2 = 0.0;
  unsigned held = 0u;
  if (t < n) {
    double x0 = inf, x1 = -inf, y0 = inf, y1 = -inf;
    for (int j = 0; j < J; ++j) {
      const double* p = pin + ((long)t * J + j) * 3;
      const double sc = p[2];
      if (sc > 0.0) {  // false for a NaN
        held |= 1u << j, S += sc;
        x0 = fmin(x0, p[0]), x1 = fmax(x1, p[0]), y0 = fmin(y0, p[1]), y1 = fmax(y1, p[1]);
      }
    }
    double s = min_size;  // as track_image (track.hip) sizes a track
    if (x1 >= x0) s = fmax(s, fmax(x1 - x0, y1 - y0));
    size2 = s * s;
  }
  S_s[t] = S, by_s[t] = -1;
  if (t < J) sig2[t] = sig.s2[t];
  __syncthreads();

  // 2. rank, and the poses in rank order
  int r = 0;
  if (t < n) {
    for (int o = 0; o < n; ++o) {
      const double So = S_s[o];
      r += (So > S || (So == S && o < t)) ? 1 : 0;
    }
    order_s[r] = t, rank_s[t] = r, hm_s[r] = held, s2_s[r] = size2;
    for (int j = 0; j < J; ++j) {
      const double* p = pin + ((long)t * J + j) * 3;
      px[j * P + r] = p[0], py[j * P + r] = p[1];
    }
  }
  __syncthreads();

  // 3. similarity
  const int nw = (n + 63) >> 6;
  for (int task = wave; task < n * nw; task += 4) {  // uniform per wave
    const int ra = task / nw, w = task - ra * nw, rb = w * 64 + lane;
    bool similar = false;
    if (rb > ra && rb < n) {
      const unsigned common = hm_s[ra] & hm_s[rb];
      const double sa2 = s2_s[ra];
      double sum = 0.0;
      int nc = 0;
      for (int j = 0; j < J; ++j)
        if ((common >> j) & 1u) {
          const double dx = px[j * P + ra] - px[j * P + rb], dy = py[j * P + ra] - py[j * P + rb];
          sum += (dx * dx + dy * dy) / (sa2 * sig2[j]);
          ++nc;
        }
      similar = nc >= min_common && nc > 0 && sum / (double)nc <= max_dist;  // false for a NaN
    }
    const unsigned long long word = __ballot(similar);
    if (lane == 0) sim[ra * 4 + w] = word;
  }
  __syncthreads();

  // 4. the sweep in rank order
  if (wave == 0) {
    unsigned long long removed = 0ull;
    for (int ra = 0; ra < n; ++ra) {
      const unsigned long long mine = __shfl(removed, ra >> 6);
      if ((mine >> (ra & 63)) & 1ull) continue;  // a suppressed person suppresses nobody (uniform)
      const unsigned long long row = lane < nw ? sim[ra * 4 + lane] : 0ull;
      const unsigned long long fresh = row & ~removed;
      removed |= fresh;
      for (int w = 0; w < nw; ++w) {
        const unsigned long long f = __shfl(fresh, w);
        if ((f >> lane) & 1ull) by_s[w * 64 + lane] = ra;
      }
    }
  }
  __syncthreads();

  // 5. compaction in input order
  const bool kept = t < n && by_s[r] < 0;
  const unsigned long long kb = __ballot(kept);
  if (lane == 0) wtot[wave] = __popcll(kb);
  __syncthreads();
  int o = __popcll(kb & ((1ull << lane) - 1ull)), total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) o += wtot[w];
    total += wtot[w];
  }
  if (kept) from_s[o] = t;
  if (t < P) {
    if (supp_by) supp_by[(long)b * P + t] = (t < n && !kept) ? order_s[by_s[r]] : -1;
    if (kept_from && t >= total) kept_from[(long)b * P + t] = -1;
  }
  if (kept && kept_from) kept_from[(long)b * P + o] = t;
  if (t == 0) n_out[b] = total;
  __syncthreads();

  double* pout = ppl_out + (long)b * P * J * 3;
  int* cout = cand_out + (long)b * P * J;
  for (int e = t; e < P * J; e += 256) {
    const int q = e / J, j = e - q * J;
    double x = 0.0, y = 0.0, sc = 0.0;
    int c = -1;
    if (q < total) {
      const int A = from_s[q];
      int src = A;
      c = cin[A * J + j];
      if (absorb && c < 0) {  // missing or filled: the first-ranked donor among the people A suppressed
        const int rA = rank_s[A];
        for (int rd = rA + 1; rd < n; ++rd) {
          if (by_s[rd] != rA) continue;
          const int d = order_s[rd], cd = cin[d * J + j];
          if (cd >= 0) {
            src = d, c = cd;
            break;
          }
        }
      }
      const double* p = pin + ((long)src * J + j) * 3;
      x = p[0], y = p[1], sc = p[2];
    }
    pout[(long)e * 3] = x, pout[(long)e * 3 + 1] = y, pout[(long)e * 3 + 2] = sc;
    cout[e] = c;
  }
}

size_t pair_cost_lds_bytes(int J, int max_det) { return ((size_t)2 * J * max_det + 6 * (size_t)max_det) * sizeof(double); }

int launch_pair_cost(const void* next, int ncp, int nc0, int ekind, int NB, int H, int W, int J, int max_det, double scale, const int* counts,
                     const double* dets, const int* lut, const double* mean, const double* stdev, double* cost, void* stream) {
  if (NB * J <= 0) return 0;
  if (max_det < 1 || max_det > kPeopleMaxDet || J > kPeopleMaxJoints) return (int)hipErrorInvalidValue;
  return people_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(pair_cost_kernel<T>, dim3(NB * J), dim3(256), pair_cost_lds_bytes(J, max_det), (hipStream_t)stream, (const T*)next, ncp,
                       nc0, H, W, J, max_det, scale, counts, dets, lut, mean, stdev, cost);
    return (int)hipGetLastError();
  });
}

int launch_assemble(int NB, int J, int max_det, int max_people, int min_joints, double max_cost, double seed_thr, const int* counts,
                    const double* dets, const double* cost, const int* order, double* link, int* n_people, double* people, int* cand,
                    void* stream) {
  if (NB <= 0 || J <= 0) return 0;
  if (max_det < 1 || max_det > kPeopleMaxDet || J > kPeopleMaxJoints || max_people < 1 || max_people > kPeopleMaxPeople)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(assemble_kernel, dim3(NB), dim3(256), (size_t)max_people * J * sizeof(int), (hipStream_t)stream, J, max_det, max_people,
                     min_joints, max_cost, seed_thr, counts, dets, cost, order, link, n_people, people, cand);
  return (int)hipGetLastError();
}

int launch_complete(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, const void* next, int ncp, int nc0,
                    int next_ekind, int NB, int H, int W, int J, int max_det, int max_people, double scale, int radius, float fill_thr,
                    int fill_radius, int min_support, const double* dets, const int* lut, const double* mean, const double* stdev,
                    const int* n_people, const int* cand_in, double* people, int* cand_out, void* stream) {
  if (NB <= 0 || J <= 0) return 0;
  if (max_det < 1 || max_det > kPeopleMaxDet || J > kPeopleMaxJoints || max_people < 1 || max_people > kPeopleMaxPeople || H < 1 || W < 1 ||
      (long)H * W > 0x7ffffffe || radius < 0 || fill_radius < 0 || fill_radius > kCompleteMaxRadius || min_support < 1)
    return (int)hipErrorInvalidValue;
  return people_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    return people_by_kind(next_ekind, [&](auto* ntag) {
      using TN = std::remove_pointer_t<decltype(ntag)>;
      hipLaunchKernelGGL((complete_kernel<T, TN>), dim3(NB * J), dim3(256), 0, (hipStream_t)stream, (const T*)prob, pcp, pc0, (const T*)loc, lcp,
                         lc0, (const TN*)next, ncp, nc0, H, W, J, max_det, max_people, scale, radius, fill_thr, fill_radius, min_support, dets,
                         lut, mean, stdev, n_people, cand_in, people, cand_out);
      return (int)hipGetLastError();
    });
  });
}

size_t dedupe_lds_bytes(int J, int max_people) { return (size_t)2 * J * max_people * sizeof(double); }

int launch_dedupe(int NB, int J, int max_people, double max_dist, int min_common, double min_size, int absorb, const double* sigma,
                  const int* n_in, const double* people_in, const int* cand_in, int* n_out, double* people_out, int* cand_out,
                  int* kept_from, int* suppressed_by, void* stream) {
  if (NB <= 0) return 0;
  if (J < 1 || J > kPeopleMaxJoints || max_people < 1 || max_people > kPeopleMaxPeople || min_common < 1) return (int)hipErrorInvalidValue;
  DedupeSigma sig;
  for (int j = 0; j < kPeopleMaxJoints; ++j) sig.s2[j] = (sigma && j < J) ? sigma[j] * sigma[j] : 1.0;
  const size_t lds = dedupe_lds_bytes(J, max_people);
  if (lds > 32 * 1024) {  // beyond what a launch gets unasked (the kernel's own arrays take 16 KiB more); 128 KiB at J = 32, P = 256
    const hipError_t e = hipFuncSetAttribute((const void*)dedupe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(dedupe_kernel, dim3(NB), dim3(256), lds, (hipStream_t)stream, J, max_people, max_dist, min_common, min_size, absorb, sig,
                     n_in, people_in, cand_in, n_out, people_out, cand_out, kept_from, suppressed_by);
  return (int)hipGetLastError();
}

}  // namespace dc
