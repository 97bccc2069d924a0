// people.cpp — bottom-up assembly of people (dc_net_assemble_people) and the reader of the pair-statistics file it is fed from
// (dc_pair_stats_read).  The kernels are in people.hip; the grouping rule is stated in include/deepcut_hip.h.
//
// PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn has no consumer of `next_pred` (it stops at the maps); only the
// label encoding of src/caffe/layers/pose_data_layer.cpp:686-802 is restated, as in the two decoders of net_image.cpp.
#include <cctype>

#include "net_internal.h"

namespace dc {

// ---- the `joint_pairs_stats` file ------------------------------------------------------------------------------------
namespace {
struct StatMatrix {
  std::string name;
  long rows = 0, cols = 0;
  std::vector<double> v;
};

struct StatTokens {
  const std::string& s;
  const std::string& path;
  size_t p = 0;
  StatTokens(const std::string& text, const std::string& file) : s(text), path(file) {}
  bool next(std::string& tok) {
    while (p < s.size() && std::isspace((unsigned char)s[p])) ++p;
    if (p >= s.size()) return false;
    const size_t b = p;
    while (p < s.size() && !std::isspace((unsigned char)s[p])) ++p;
    tok.assign(s, b, p - b);
    return true;
  }
  [[noreturn]] void bad(const std::string& what) const { throw DcError(DC_EINVAL, "pair statistics " + path + ": " + what); }
  double number(const std::string& tok, const std::string& where) const {
    char* end = nullptr;
    const double v = std::strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end) bad("'" + tok + "' is not a number (" + where + ")");
    return v;
  }
  long dimension(const std::string& where) {
    std::string tok;
    if (!next(tok)) bad("truncated block: " + where + " has no size line");
    const double v = number(tok, "size of " + where);
    if (!(v >= 0 && v <= 1e6 && v == std::floor(v))) bad("size '" + tok + "' of " + where + " is not a whole number of rows / columns");
    return (long)v;
  }
};
}  // namespace

PairStats read_pair_stats(const std::string& path) {
  const std::string text = read_file(path);
  StatTokens tk(text, path);
  std::vector<StatMatrix> mats;
  std::string tok;
  while (mats.size() < 3 && tk.next(tok)) {
    StatMatrix m;
    if (tok != "#") tk.bad("expected '# <name>' in front of matrix " + std::to_string(mats.size()) + ", found '" + tok + "'");
    if (!tk.next(m.name)) tk.bad("truncated block: '#' without a matrix name");
    const std::string where = "matrix " + std::to_string(mats.size()) + " ('" + m.name + "')";
    m.rows = tk.dimension(where);
    m.cols = tk.dimension(where);
    m.v.reserve((size_t)(m.rows * m.cols));
    for (long i = 0; i < m.rows * m.cols; ++i) {
      if (!tk.next(tok))
        tk.bad("truncated block: " + where + " holds " + std::to_string(i) + " of " + std::to_string(m.rows * m.cols) + " numbers");
      m.v.push_back(tk.number(tok, where));
    }
    mats.push_back(std::move(m));
  }
  if (mats.size() < 3)
    tk.bad("fewer than three matrices (edges, means, standard deviations): found " + std::to_string(mats.size()));
  for (size_t i = 0; i < 3; ++i)
    if (mats[i].cols != 2)
      tk.bad("matrix " + std::to_string(i) + " ('" + mats[i].name + "') is " + std::to_string(mats[i].rows) + " x " +
             std::to_string(mats[i].cols) + ", not E x 2");
  for (size_t i = 1; i < 3; ++i)
    if (mats[i].rows != mats[0].rows)
      tk.bad("differing row counts: " + std::to_string(mats[0].rows) + " edges, but matrix " + std::to_string(i) + " ('" + mats[i].name +
             "') has " + std::to_string(mats[i].rows) + " rows");
  PairStats st;
  const size_t n = (size_t)mats[0].rows * 2;
  st.edges.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const double c = mats[0].v[i];
    if (!(c >= 1 && c <= 1e6 && c == std::floor(c)))
      tk.bad("edge " + std::to_string(i / 2) + ": class id " + std::to_string(c) + " is not a whole number >= 1 (class ids are 1-based)");
    st.edges[i] = (int)c - 1;
  }
  for (size_t i = 0; i < n; ++i) {
    if (!std::isfinite(mats[1].v[i])) tk.bad("edge " + std::to_string(i / 2) + ": mean is not finite");
    const double s = mats[2].v[i];
    if (!(std::isfinite(s) && s > 0))
      tk.bad("edge " + std::to_string(i / 2) + ": standard deviation " + std::to_string(s) + " is not positive and finite");
  }
  st.mean = std::move(mats[1].v);
  st.stdev = std::move(mats[2].v);
  return st;
}

// ---- the device path ---------------------------------------------------------------------------------------------------
// Stage A = Net::detect_parts' launch with its outputs left in the scratch buffer, stage B = launch_pair_cost, stage C =
// launch_assemble, stage D = launch_complete (only with completion enabled: dc_net_set_completion), stage E = launch_dedupe (only with
// duplicate suppression enabled: dc_net_set_dedupe): three to five launches on one stream with nothing in between
// (DC_OPT_SPARSE_PAIRWISE on a net without next_pred: the sparse head's two launches between A and B, sparse_pairwise.cpp), then the
// downloads of the results.  The argument checks and the device half are functions of their own: NetGroup::assemble_people runs them
// on the fused maps of a pyramid (net_group.cpp).
void Net::check_assemble_params(const AssembleParams& q) {
  auto bad = [](const std::string& m) { throw DcError(DC_EINVAL, "assemble_people: " + m); };
  if (!(q.scale > 0) || !std::isfinite(q.scale)) bad("scale must be positive");
  if (!(q.threshold >= 0.f)) bad("threshold must be >= 0");
  if (q.radius < 0 || q.radius > 64) bad("radius must be in [0, 64]");
  if (q.max_det < 1 || q.max_det > kPeopleMaxDet) bad("max_det must be in [1, " + std::to_string(kPeopleMaxDet) + "]");
  if (!(q.max_cost >= 0) || !std::isfinite(q.max_cost)) bad("max_cost must be finite and >= 0");
  if (!std::isfinite(q.seed_threshold)) bad("seed_threshold must be finite");
  if (q.max_people < 1 || q.max_people > kPeopleMaxPeople) bad("max_people must be in [1, " + std::to_string(kPeopleMaxPeople) + "]");
}

// dc_net_set_completion / dc_group_set_completion: refused here, with no device, so that no assembling entry has to
CompleteParams CompleteParams::checked(const dc_complete_params* p) {
  CompleteParams c;
  if (!p || !p->enabled) return c;  // off: the other fields are not read
  auto bad = [](const std::string& m) { throw DcError(DC_EINVAL, "set_completion: " + m); };
  if (!std::isfinite(p->fill_threshold) || !(p->fill_threshold > 0.f)) bad("fill_threshold must be finite and > 0");
  if (p->fill_radius < 0 || p->fill_radius > kCompleteMaxRadius) bad("fill_radius must be in [0, " + std::to_string(kCompleteMaxRadius) + "]");
  if (p->min_support < 1) bad("min_support must be >= 1");
  c.enabled = 1;
  c.fill_threshold = p->fill_threshold;
  c.fill_radius = p->fill_radius;
  c.min_support = p->min_support;
  return c;
}

// dc_net_set_dedupe / dc_group_set_dedupe / dc_dedupe_people: likewise
DedupeParams DedupeParams::checked(const dc_dedupe_params* p, const char* who, bool always) {
  DedupeParams d;
  if (!always && (!p || !p->enabled)) return d;  // off: the other fields are not read
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  if (!p) bad("null argument: params");
  if (!std::isfinite(p->max_dist) || !(p->max_dist >= 0)) bad("max_dist must be finite and >= 0");
  if (p->min_common < 1) bad("min_common must be >= 1");
  if (!std::isfinite(p->min_size) || !(p->min_size > 0)) bad("min_size must be finite and > 0");
  if (p->n_sigma < 0 || p->n_sigma > kPeopleMaxJoints) bad("n_sigma must be in [0, " + std::to_string(kPeopleMaxJoints) + "]");
  if (p->n_sigma != 0 && !p->sigma) bad("sigma must be [n_sigma] values, or NULL with n_sigma = 0");
  for (int j = 0; j < p->n_sigma; ++j)
    if (!(std::isfinite(p->sigma[j]) && p->sigma[j] > 0)) bad("sigma of joint " + std::to_string(j) + " must be finite and > 0");
  if (p->absorb != 0 && p->absorb != 1) bad("absorb must be 0 or 1");
  d.enabled = 1;
  d.max_dist = p->max_dist, d.min_size = p->min_size;
  d.min_common = p->min_common, d.n_sigma = p->n_sigma, d.absorb = p->absorb;
  for (int j = 0; j < p->n_sigma; ++j) d.sigma[j] = p->sigma[j];
  return d;
}

void DedupeParams::check_joints(const char* who, int J) const {
  if (n_sigma != 0 && n_sigma != J)
    throw DcError(DC_ESHAPE, std::string(who) + ": dedupe holds " + std::to_string(n_sigma) + " sigma values (n_sigma), the poses " +
                                 std::to_string(J) + " joints");
  if (min_common > J)
    throw DcError(DC_ESHAPE, std::string(who) + ": dedupe min_common = " + std::to_string(min_common) + " is more than the poses' " +
                                 std::to_string(J) + " joints");
}

// dc_dedupe_people: stage E alone on host poses (top-down poses before dc_tracker_update).  One launch on the utility stream, synchronous
void dedupe_people(const dc_dedupe_params* params, int nb, int P, int J, const int* n_people, const double* people, const int* cand,
                   int* n_out, double* people_out, int* cand_out, int* kept_from, int* suppressed_by) {
  const char* who = "dedupe_people";
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  const DedupeParams d = DedupeParams::checked(params, who, true);
  if (nb < 1) bad("nb must be >= 1");
  if (P < 1 || P > kPeopleMaxPeople) bad("max_people (P) must be in [1, " + std::to_string(kPeopleMaxPeople) + "]");
  if (J < 1 || J > kPeopleMaxJoints) bad("n_joints (J) must be in [1, " + std::to_string(kPeopleMaxJoints) + "]");
  for (int b = 0; b < nb; ++b)
    if (n_people[b] < 0 || n_people[b] > P)
      bad("n_people[" + std::to_string(b) + "] = " + std::to_string(n_people[b]) + " is outside [0, P = " + std::to_string(P) + "]");
  d.check_joints(who, J);
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "dedupe_people() in CPU mode");
  if (device_count() <= 0) throw DcError(DC_EDEVICE, "no HIP device visible");
  HIPCHECK(hipSetDevice(Context::get().device));
  const size_t img = (size_t)P * J, N = (size_t)nb;
  // without `cand` a joint counts as assigned exactly when it is held: candidate 0 there, -1 elsewhere
  std::vector<int> made;
  if (!cand) {
    made.assign(N * img, -1);
    for (int b = 0; b < nb; ++b)
      for (size_t e = 0; e < (size_t)n_people[b] * J; ++e)
        if (people[((size_t)b * img + e) * 3 + 2] > 0.0) made[(size_t)b * img + e] = 0;
    cand = made.data();
  }
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t np_b = up(N * sizeof(int)), ppl_b = up(N * img * 3 * sizeof(double)), cand_b = up(N * img * sizeof(int)),
               row_b = up(N * P * sizeof(int));
  RuntimeLock rl;
  hipStream_t s = util_stream();
  DevBuf buf;
  unsigned char* at = (unsigned char*)buf.get(2 * (np_b + ppl_b + cand_b + row_b));
  auto take = [&](size_t b) {
    unsigned char* r = at;
    at += b;
    return r;
  };
  int* d_np = (int*)take(np_b);
  double* d_ppl = (double*)take(ppl_b);
  int* d_cand = (int*)take(cand_b);
  int* d_np2 = (int*)take(np_b);
  double* d_ppl2 = (double*)take(ppl_b);
  int* d_cand2 = (int*)take(cand_b);
  int* d_from = (int*)take(row_b);
  int* d_by = (int*)take(row_b);
  HIPCHECK(hipMemcpyAsync(d_np, n_people, N * sizeof(int), hipMemcpyHostToDevice, s));
  // only the people that exist are read on either side
  for (int b = 0; b < nb; ++b)
    if (n_people[b] > 0) {
      const size_t m = (size_t)n_people[b] * J;
      HIPCHECK(hipMemcpyAsync(d_ppl + (size_t)b * img * 3, people + (size_t)b * img * 3, m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHECK(hipMemcpyAsync(d_cand + (size_t)b * img, cand + (size_t)b * img, m * sizeof(int), hipMemcpyHostToDevice, s));
    }
  KCHECK(launch_dedupe(nb, J, P, d.max_dist, d.min_common, d.min_size, d.absorb, d.sigma_or_null(), d_np, d_ppl, d_cand, d_np2, d_ppl2, d_cand2,
                       d_from, d_by, s));
  HIPCHECK(hipMemcpyAsync(n_out, d_np2, N * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(people_out, d_ppl2, N * img * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (cand_out) HIPCHECK(hipMemcpyAsync(cand_out, d_cand2, N * img * sizeof(int), hipMemcpyDeviceToHost, s));
  if (kept_from) HIPCHECK(hipMemcpyAsync(kept_from, d_from, N * P * sizeof(int), hipMemcpyDeviceToHost, s));
  if (suppressed_by) HIPCHECK(hipMemcpyAsync(suppressed_by, d_by, N * P * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
}

std::vector<int> Net::check_assemble_graph(const AssembleParams& q, int J, int n_edges, const int* edges, const double* mean,
                                           const double* stdev, const int* joint_order) {
  auto bad = [](const std::string& m) { throw DcError(DC_EINVAL, "assemble_people: " + m); };
  if (J < 1 || J > kPeopleMaxJoints)
    throw DcError(DC_ESHAPE, "assemble_people: " + std::to_string(J) + " joints, the assembly holds up to " + std::to_string(kPeopleMaxJoints));
  if (q.min_joints < 1 || q.min_joints > J) bad("min_joints must be in [1, " + std::to_string(J) + "]");
  if (n_edges < 0) bad("n_edges must be >= 0");
  // the lookup table of both directions: lut[a*J + c] = the lowest edge index whose (joint, next joint) is (a, c)
  std::vector<int> table((size_t)J * J + J, -1);
  for (int l = 0; l < n_edges; ++l) {
    const int a = edges[2 * l], c = edges[2 * l + 1];
    if (a < 0 || a >= J || c < 0 || c >= J)
      bad("edge " + std::to_string(l) + " (" + std::to_string(a) + ", " + std::to_string(c) + ") names a joint outside [0, " + std::to_string(J) + ")");
    if (a == c) bad("edge " + std::to_string(l) + " joins joint " + std::to_string(a) + " to itself");
    if (table[(size_t)a * J + c] < 0) table[(size_t)a * J + c] = l;
  }
  int* order = table.data() + (size_t)J * J;
  {
    std::vector<char> seen(J, 0);
    for (int i = 0; i < J; ++i) {
      const int j = joint_order ? joint_order[i] : i;
      if (j < 0 || j >= J || seen[j]) bad("joint_order is not a permutation of 0.." + std::to_string(J - 1) + " (entry " + std::to_string(i) + ")");
      seen[j] = 1;
      order[i] = j;
    }
  }
  for (int i = 0; i < 2 * n_edges; ++i) {
    if (mean && !std::isfinite(mean[i])) bad("mean of edge " + std::to_string(i / 2) + " is not finite");
    if (stdev && !(std::isfinite(stdev[i]) && stdev[i] > 0)) bad("std of edge " + std::to_string(i / 2) + " is not positive and finite");
  }
  return table;
}

void Net::assemble_people(const AssembleParams& q, int n_edges, const int* edges, const double* mean, const double* stdev,
                          const int* joint_order, int* n_people, double* people, int* cand, double* cost, Tracker* tracker, long long* ids,
                          int* place, const int* slot_of) {
  check_assemble_params(q);
  const std::vector<int>& pshape = prob_shape();
  const std::vector<int> table = check_assemble_graph(q, pshape[1], n_edges, edges, mean, stdev, joint_order);
  if (tracker) tracker->check_call("track_people", pshape[0], q.max_people, pshape[1], slot_of);
  // (the arguments above are refused with or without a device; from here on the device is needed)
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "assemble_people() in CPU mode");
  ensure_device();
  const MapRef P = map_ref("prob");
  // the tracker's launch behind stage C: the runtime lock is taken there and kept until assemble_maps has waited for the stream
  std::unique_lock<std::recursive_mutex> order(runtime_mu(), std::defer_lock);
  AfterPeople after;
  if (tracker)
    after = [&](const int* d_np, const double* d_ppl, const int* d_cand) {
      order.lock();
      tracker->prepare(device, P.NB, stream);
      tracker->wait_done();
      return tracker->enqueue_chained(P.NB, q.max_people, slot_of, d_np, d_ppl, d_cand, ids, place, people, cand, stream);
    };
  assemble_last(q, table, n_edges, mean, stdev, n_people, people, cand, cost, after, true);
}

// the device half of assemble_people / track_frames_async on the maps of the net's last (enqueued) forward
void Net::assemble_last(const AssembleParams& q_in, const std::vector<int>& table, int n_edges, const double* mean, const double* stdev,
                        int* n_people, double* people, int* cand, double* cost, const AfterPeople& after,
                        bool wait) {
  AssembleParams q = q_in;
  q.complete = completion;  // stage D, when the net has it enabled
  q.dedupe = dedupe;        // stage E likewise
  const MapRef P = map_ref("prob"), L = map_ref("loc_pred");
  if (sparse_pairwise && !next_in_plan()) {  // DC_OPT_SPARSE_PAIRWISE: the head at the candidates' cells, between stages A and B
    const SparseNext sn = sparse_next(P.NB * P.C * q.max_det, 0);
    assemble_maps(P, L, sn.N, q, table, n_edges, mean, stdev, [this](size_t bytes) { return scratch(bytes); }, stream, n_people, people, cand, cost,
                  [&](const int* d_cnt, const double* d_det) {
                    KCHECK(launch_sparse_head(sn.a, sn.ekind, d_cnt, d_det, P.C, q.max_det, nullptr, P.NB * P.C * q.max_det, sn.work, stream));
                  },
                  after, &asm_tables_, wait);
    return;
  }
  const MapRef N = map_ref("next_pred");
  assemble_maps(P, L, N, q, table, n_edges, mean, stdev, [this](size_t bytes) { return scratch(bytes); }, stream, n_people, people, cand, cost,
                nullptr, after, &asm_tables_, wait);
}

void Net::track_frames_async(Tracker* tracker, const dc_frame* frames, const unsigned char* bgr, int n, int h, int w, double scale,
                             bool is_device, const int* slot_of, const AssembleParams& p, int n_edges, const int* edges, const double* mean,
                             const double* stdev, const int* joint_order, int* n_people, double* people, int* cand, long long* ids,
                             int* place, const OverlayArgs* overlay) {
  const char* who = "track_frames_async";
  // what forward_images refuses ...
  if (frames) check_frames(who, frames, n, h, w);
  // ... what assemble_people refuses (the batch of the forward to come is n; the joints do not depend on it) ...
  check_assemble_params(p);
  const std::vector<int>& pshape = prob_shape();
  const std::vector<int> table = check_assemble_graph(p, pshape[1], n_edges, edges, mean, stdev, joint_order);
  // ... and what the tracker refuses
  if (tracker) tracker->check_call(who, n, p.max_people, pshape[1], slot_of);
  else if (ids) throw DcError(DC_EINVAL, "track_frames_async: ids without a tracker (ids must be NULL when tracker is NULL)");
  // ... and what the overlays refuse, in the words of dc_draw_people and dc_redact_people
  std::unique_ptr<OverlayPlan> plan;
  if (overlay && overlay->any()) {
    check_frame_dims(who, n, h, w);
    check_people_dims(who, p.max_people, pshape[1]);
    dc_frame packed{};
    packed.format = DC_PIX_BGR24;
    plan.reset(new OverlayPlan(who, frames ? frames[0] : packed, n, h, w, p.max_people, pshape[1], *overlay, tracker != nullptr));
  }
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "track_frames_async() in CPU mode");
  prep_images(bgr, n, h, w, scale, is_device, nullptr, false, frames);
  enqueue_plan(stream);
  AfterPeople after;
  if (!plan) {
    if (tracker)
      after = [&](const int* d_np, const double* d_ppl, const int* d_cand) {
        RuntimeLock rl;  // for the enqueue only: the tracker's event keeps the order from here on
        tracker->prepare(device, n, stream);
        return tracker->enqueue_chained(n, p.max_people, slot_of, d_np, d_ppl, d_cand, ids, place, people, cand, stream);
      };
  } else {
    after = [&](const int* d_np, const double* d_ppl, const int* d_cand) {
      unsigned char* block = (unsigned char*)overlay_dev_.get(plan->bytes);
      int* d_redacted = reinterpret_cast<int*>(block + plan->at_redacted);
      bool delivered = false;
      if (tracker) {
        // the builders read the people, cand and ids the update leaves in the tracker's shared scratch: in front of its event
        const Tracker::BeforeDone build = [&](const double* t_ppl, const int* t_cand, const long long* t_ids) {
          plan->build(block, n, d_np, t_ppl, t_cand, t_ids, d_redacted, stream);
        };
        RuntimeLock rl;  // for the enqueue only: the tracker's event keeps the order from here on
        tracker->prepare(device, n, stream);
        delivered = tracker->enqueue_chained(n, p.max_people, slot_of, d_np, d_ppl, d_cand, ids, place, people, cand, stream, &build);
      } else {
        plan->build(block, n, d_np, d_ppl, cand ? d_cand : nullptr, nullptr, d_redacted, stream);
      }
      // the tile kernels read the net's own block: behind the event.  Host pixels were staged by the pre-processing and are written there
      hipStream_t s = (hipStream_t)stream;
      std::vector<DrawPlanes> planes((size_t)n);
      const size_t image = (size_t)h * w * 3;
      for (int b = 0; b < n; ++b) {
        if (frames) {
          const FramePlanes& f = frame_host_[(size_t)b];
          planes[(size_t)b] = DrawPlanes{const_cast<unsigned char*>(f.plane0), const_cast<unsigned char*>(f.plane1), f.pitch0, f.pitch1};
        } else {
          unsigned char* base = is_device ? const_cast<unsigned char*>(bgr) : img_dev_.dev;
          planes[(size_t)b] = DrawPlanes{base + image * b, nullptr, 3 * w, 0};
        }
      }
      plan->tiles(block, planes.data(), n, stream);
      if (!is_device) {  // every host frame travels back (which of them is touched is known on the device only), never its padding
        if (!frames) HIPCHECK(hipMemcpyAsync(const_cast<unsigned char*>(bgr), img_dev_.dev, image * n, hipMemcpyDeviceToHost, s));
        for (int b = 0; frames && b < n; ++b) {
          const DrawPlanes& d = planes[(size_t)b];
          const bool nv12 = frames[b].format == DC_PIX_NV12;
          HIPCHECK(hipMemcpy2DAsync(const_cast<void*>(frames[b].plane[0]), (size_t)frames[b].pitch[0], d.plane0, (size_t)d.pitch0,
                                    (size_t)d.pitch0, (size_t)h, hipMemcpyDeviceToHost, s));
          if (nv12)
            HIPCHECK(hipMemcpy2DAsync(const_cast<void*>(frames[b].plane[1]), (size_t)frames[b].pitch[1], d.plane1, (size_t)d.pitch1,
                                      (size_t)d.pitch1, (size_t)((h + 1) / 2), hipMemcpyDeviceToHost, s));
        }
      }
      if (plan->redact && overlay->redacted)
        HIPCHECK(hipMemcpyAsync(overlay->redacted, d_redacted, (size_t)n * p.max_people * sizeof(int), hipMemcpyDeviceToHost, s));
      return delivered;
    };
  }
  assemble_last(p, table, n_edges, mean, stdev, n_people, people, cand, nullptr, after, false);
}

void Net::assemble_maps(const MapRef& P, const MapRef& L, const MapRef& N, const AssembleParams& q, const std::vector<int>& table, int n_edges,
                        const double* mean, const double* stdev, const std::function<void*(size_t)>& scratch, void* stream, int* n_people,
                        double* people, int* cand, double* cost, const std::function<void(const int*, const double*)>& between,
                        const AfterPeople& after, AssembleTables* keep, bool wait) {
  const int J = P.C;
  if (L.C != 2 * P.C || L.H != P.H || L.W != P.W || L.NB != P.NB || L.es != P.es)
    throw DcError(DC_ESHAPE, "assemble_people: loc_pred must have 2 channels per joint and the score map's size");
  if (N.H != P.H || N.W != P.W || N.NB != P.NB) throw DcError(DC_ESHAPE, "assemble_people: next_pred must have the score map's size");
  if (N.C % 2 || n_edges != N.C / 2)
    throw DcError(DC_ESHAPE, "assemble_people: " + std::to_string(n_edges) + " edges for a next_pred of " + std::to_string(N.C) +
                                 " channels (2 per regression edge)");
  const bool dedupe = q.dedupe.enabled != 0;
  if (dedupe) q.dedupe.check_joints("assemble_people", J);
  const int NB = P.NB, MD = q.max_det, PP = q.max_people, E = n_edges, lists = NB * J;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t cnt_b = up((size_t)lists * sizeof(int));
  const size_t spill_b = up((size_t)lists * P.H * P.W * sizeof(unsigned long long));
  const size_t det_b = up((size_t)lists * MD * 5 * sizeof(double));
  if (!wait && !keep) throw DcError(DC_EINVAL, "assemble_people: the no-wait form needs its tables kept");
  const size_t tab_b = up(table.size() * sizeof(int));
  const size_t st_b = up((size_t)std::max(E, 1) * 4 * sizeof(double));
  const size_t cost_b = up((size_t)NB * J * J * MD * MD * sizeof(double));
  const size_t link_b = up((size_t)NB * PP * MD * sizeof(double));
  const size_t np_b = up((size_t)NB * sizeof(int));
  const size_t ppl_b = up((size_t)NB * PP * J * 3 * sizeof(double));
  const size_t cand_b = up((size_t)NB * PP * J * sizeof(int));
  const bool complete = q.complete.enabled != 0;
  const size_t fill_b = complete ? cand_b : 0;  // stage D writes `cand` into a buffer of its own: it reads stage C's while it runs
  const size_t kept_b = dedupe ? np_b + ppl_b + cand_b : 0;  // stage E writes all three into buffers of its own, for the same reason
  unsigned char* base =
      (unsigned char*)scratch(cnt_b + spill_b + det_b + (keep ? 0 : tab_b + st_b) + cost_b + link_b + np_b + ppl_b + cand_b + fill_b + kept_b);
  unsigned char* at = base;
  auto take = [&](size_t b) {
    unsigned char* r = at;
    at += b;
    return r;
  };
  int* d_cnt = (int*)take(cnt_b);
  unsigned long long* d_spill = (unsigned long long*)take(spill_b);
  double* d_det = (double*)take(det_b);
  hipStream_t s = (hipStream_t)stream;
  std::vector<double> stats((size_t)4 * E);
  for (int i = 0; i < 2 * E; ++i) stats[i] = mean ? mean[i] : 0.0, stats[(size_t)2 * E + i] = stdev ? stdev[i] : 1.0;
  int* d_tab;
  double* d_mean;
  if (keep) {
    std::vector<unsigned char> now(tab_b + st_b, 0);
    std::memcpy(now.data(), table.data(), table.size() * sizeof(int));
    if (E) std::memcpy(now.data() + tab_b, stats.data(), stats.size() * sizeof(double));
    bool same = keep->buf.dev && keep->stream == stream && keep->host == now;
    if (keep->buf.reserve(now.size())) same = false;
    if (!same) {
      // rare (another graph, other statistics): what is in flight on this stream may still read the old content, and an upload from the
      // host copy may not have read it yet — both are waited for before either is replaced
      HIPCHECK(hipStreamSynchronize(s));
      keep->host.swap(now);
      HIPCHECK(hipMemcpyAsync(keep->buf.dev, keep->host.data(), keep->host.size(), hipMemcpyHostToDevice, s));
      keep->stream = stream;
    }
    d_tab = (int*)keep->buf.dev;
    d_mean = (double*)(keep->buf.dev + tab_b);
  } else {
    d_tab = (int*)take(tab_b);
    d_mean = (double*)take(st_b);
  }
  double* d_std = d_mean + (size_t)2 * E;
  double* d_cost = (double*)take(cost_b);
  double* d_link = (double*)take(link_b);
  int* d_np = (int*)take(np_b);
  double* d_ppl = (double*)take(ppl_b);
  int* d_cand = (int*)take(cand_b);
  int* d_filled = complete ? (int*)take(fill_b) : nullptr;
  int* d_np_kept = dedupe ? (int*)take(np_b) : nullptr;
  double* d_ppl_kept = dedupe ? (double*)take(ppl_b) : nullptr;
  int* d_cand_kept = dedupe ? (int*)take(cand_b) : nullptr;
  if (!keep) {
    HIPCHECK(hipMemcpyAsync(d_tab, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (E) HIPCHECK(hipMemcpyAsync(d_mean, stats.data(), stats.size() * sizeof(double), hipMemcpyHostToDevice, s));
  }
  KCHECK(launch_part_select(P.ptr, P.cp, P.c0, L.ptr, L.cp, L.c0, P.ek, NB, P.H, P.W, J, q.threshold, q.radius, q.scale, MD, d_spill, d_cnt,
                            d_det, stream));
  if (between) between(d_cnt, d_det);
  KCHECK(launch_pair_cost(N.ptr, N.cp, N.c0, N.ek, NB, N.H, N.W, J, MD, q.scale, d_cnt, d_det, d_tab, d_mean, d_std, d_cost, stream));
  KCHECK(launch_assemble(NB, J, MD, PP, q.min_joints, q.max_cost, (double)q.seed_threshold, d_cnt, d_det, d_cost, d_tab + (size_t)J * J, d_link,
                         d_np, d_ppl, d_cand, stream));
  if (complete) {  // stage D: the joints people lack, from the maps stages A and B read; the tracker below receives the completed people
    KCHECK(launch_complete(P.ptr, P.cp, P.c0, L.ptr, L.cp, L.c0, P.ek, N.ptr, N.cp, N.c0, N.ek, NB, P.H, P.W, J, MD, PP, q.scale, q.radius,
                           q.complete.fill_threshold, q.complete.fill_radius, q.complete.min_support, d_det, d_tab, d_mean, d_std, d_np, d_cand,
                           d_ppl, d_filled, stream));
    d_cand = d_filled;
  }
  if (dedupe) {  // stage E: the people a better one is the same as leave; the tracker and the downloads below take what it kept
    KCHECK(launch_dedupe(NB, J, PP, q.dedupe.max_dist, q.dedupe.min_common, q.dedupe.min_size, q.dedupe.absorb, q.dedupe.sigma_or_null(), d_np,
                         d_ppl, d_cand, d_np_kept, d_ppl_kept, d_cand_kept, nullptr, nullptr, stream));
    d_np = d_np_kept, d_ppl = d_ppl_kept, d_cand = d_cand_kept;
  }
  // a tracker with smoothing on delivers people and cand itself, from step 8's outputs (the device copies here stay raw)
  const bool delivered = after ? after(d_np, d_ppl, d_cand) : false;
  HIPCHECK(hipMemcpyAsync(n_people, d_np, (size_t)NB * sizeof(int), hipMemcpyDeviceToHost, s));
  if (!delivered) HIPCHECK(hipMemcpyAsync(people, d_ppl, (size_t)NB * PP * J * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (cand && !delivered) HIPCHECK(hipMemcpyAsync(cand, d_cand, (size_t)NB * PP * J * sizeof(int), hipMemcpyDeviceToHost, s));
  if (cost) HIPCHECK(hipMemcpyAsync(cost, d_cost, (size_t)NB * J * J * MD * MD * sizeof(double), hipMemcpyDeviceToHost, s));
  if (wait) HIPCHECK(hipStreamSynchronize(s));
}

}  // namespace dc
