// track.cpp — the tracker object behind dc_tracker_*: argument checks, the device buffer of the slots' tracks and the launches of
// track.hip.  The rule is stated in include/deepcut_hip.h (dc_tracker_update).
//
// PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker; the rule is this project's own.
#include "net_internal.h"

namespace dc {

namespace {
[[noreturn]] void bad(const std::string& who, const std::string& m) { throw DcError(DC_EINVAL, who + ": " + m); }
size_t up256(size_t b) { return (b + 255) / 256 * 256; }
// the calling thread's current device for the length of a call on a tracker bound to another one (state, reset)
struct DeviceScope {
  int before = -1;
  explicit DeviceScope(int d) {
    HIPCHECK(hipGetDevice(&before));
    if (before != d) HIPCHECK(hipSetDevice(d));
    else before = -1;
  }
  ~DeviceScope() {
    if (before >= 0) (void)hipSetDevice(before);
  }
};
}  // namespace

Tracker* Tracker::create(int slots, int max_tracks, int n_joints, const double* sigma, int max_misses, int min_common, double max_dist,
                         double min_size, int motion) {
  const std::string who = "tracker_create";
  if (slots < 1 || slots > 64) bad(who, "slots must be in [1, 64]");
  if (max_tracks < 1 || max_tracks > kPeopleMaxPeople) bad(who, "max_tracks must be in [1, " + std::to_string(kPeopleMaxPeople) + "]");
  if (n_joints < 1 || n_joints > kPeopleMaxJoints) bad(who, "n_joints must be in [1, " + std::to_string(kPeopleMaxJoints) + "]");
  for (int j = 0; sigma && j < n_joints; ++j)
    if (!(std::isfinite(sigma[j]) && sigma[j] > 0)) bad(who, "sigma of joint " + std::to_string(j) + " must be finite and > 0");
  if (max_misses < 0) bad(who, "max_misses must be >= 0");
  if (min_common < 1 || min_common > n_joints) bad(who, "min_common must be in [1, " + std::to_string(n_joints) + "]");
  if (!(max_dist >= 0) || !std::isfinite(max_dist)) bad(who, "max_dist must be finite and >= 0");
  if (!(min_size > 0) || !std::isfinite(min_size)) bad(who, "min_size must be finite and > 0");
  if (motion != 0 && motion != 1) bad(who, "motion must be 0 or 1");
  std::unique_ptr<Tracker> t(new Tracker());
  t->tp = TrackParams{max_tracks, n_joints, max_misses, min_common, motion, max_dist, min_size, DC_TRACK_ASSIGN_GREEDY};
  t->slots = slots;
  t->sig2.resize((size_t)n_joints);
  for (int j = 0; j < n_joints; ++j) t->sig2[(size_t)j] = sigma ? sigma[j] * sigma[j] : 1.0;
  const size_t S = (size_t)slots, J = (size_t)n_joints;
  t->slot_stride = up256(track_slot_bytes(max_tracks, n_joints));
  t->off_sig = S * t->slot_stride;
  t->total = t->off_sig + up256(J * sizeof(double));
  return t.release();
}

Tracker::~Tracker() {
  if (done) {  // an update enqueued by an asynchronous entry may still be running on these buffers
    int before = -1;
    const bool moved = hipGetDevice(&before) == hipSuccess && before != device && hipSetDevice(device) == hipSuccess;
    (void)hipEventSynchronize((hipEvent_t)done);
    (void)hipEventDestroy((hipEvent_t)done);
    if (moved) (void)hipSetDevice(before);
  }
  dev_free(img_dev);
  dev_free(filt_dev);
  dev_free(app_dev);
  dev_free(dev);
}

void Tracker::wait_done() {
  if (done) HIPCHECK(hipEventSynchronize((hipEvent_t)done));
}

void Tracker::check_call(const char* who, int nb, int P, int J, const int* slot_of) const {
  if (slot_of) {
    if (nb < 1 || nb > kTrackMaxImages)
      bad(who, std::to_string(nb) + " images with a slot map (nb must be in [1, " + std::to_string(kTrackMaxImages) + "])");
    for (int b = 0; b < nb; ++b)
      if (slot_of[b] < 0 || slot_of[b] >= slots)
        bad(who, "slot_of[" + std::to_string(b) + "] = " + std::to_string(slot_of[b]) + " is outside [0, slots = " + std::to_string(slots) + ")");
  } else if (nb < 1 || nb > slots) {
    bad(who, std::to_string(nb) + " images for a tracker of " + std::to_string(slots) + " slots (nb must be in [1, slots])");
  }
  if (P < 1 || P > kPeopleMaxPeople) bad(who, "max_people (P) must be in [1, " + std::to_string(kPeopleMaxPeople) + "]");
  if (J != tp.J)
    throw DcError(DC_ESHAPE, std::string(who) + ": the tracker holds " + std::to_string(tp.J) + " joints (n_joints), the poses " + std::to_string(J));
}

void Tracker::prepare(int on_device, int nb, void* stream) {
  if (device >= 0 && device != on_device)
    throw DcError(DC_EDEVICE, "tracker: bound to device " + std::to_string(device) + ", used on device " + std::to_string(on_device));
  if (!dev) {
    dev_alloc((void**)&dev, total);
    device = on_device;
    dev_zero(dev, total, stream);
    dev_upload(dev + off_sig, sig2.data(), sig2.size() * sizeof(double), stream);
    hipEvent_t ev = nullptr;
    HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    done = ev;
    HIPCHECK(hipEventRecord(ev, (hipStream_t)stream));  // the next update, on whichever stream, runs behind the zeroing
  }
  const bool on = smooth.enabled != 0;
  if (on && (!filt_dev || filt_clear)) {  // the first update with smoothing on, or the first since it went from off to on: empty filters
    const size_t bytes = (size_t)slots * tp.T * tp.J * sizeof(TrackFilter);
    if (!filt_dev) dev_alloc((void**)&filt_dev, bytes);
    dev_zero(filt_dev, bytes, stream);  // set_smoothing waited for the updates before; the launch follows on this stream
    filt_clear = false;
  }
  const bool app = appear.enabled != 0;
  if (app && (!app_dev || app_clear)) {  // likewise: empty models and galleries
    app_stride = up256(track_appear_bytes(tp.T));
    const size_t bytes = (size_t)slots * app_stride;
    if (!app_dev) dev_alloc((void**)&app_dev, bytes);
    dev_zero(app_dev, bytes, stream);
    app_clear = false;
  }
  if (nb > img_cap || (on && !img_smooth) || (app && !img_appear)) {
    wait_done();  // nobody reads the old scratch any more
    const size_t N = (size_t)std::max(std::max(nb, img_cap), slots), T = (size_t)tp.T, J = (size_t)tp.J, PM = (size_t)kPeopleMaxPeople;
    size_t at = 0;
    auto take = [&](size_t bytes) {
      const size_t r = at;
      at += up256(bytes);
      return r;
    };
    const size_t o_dist = take(N * T * PM * sizeof(double)), o_np = take(N * sizeof(int)), o_ppl = take(N * PM * J * 3 * sizeof(double)),
                 o_ids = take(N * PM * sizeof(long long)), o_place = take(N * PM * sizeof(int));
    const bool with = on || img_smooth;
    const size_t o_smooth = with ? take(N * PM * J * 3 * sizeof(double)) : 0, o_src = with ? take(N * PM * J * sizeof(int)) : 0,
                 o_cand = with ? take(N * PM * J * sizeof(int)) : 0;
    const bool with_app = app || img_appear;
    const size_t o_desc = with_app ? take(N * PM * kTrackModel * sizeof(int)) : 0, o_qdesc = with_app ? take(N * PM * kTrackModel * sizeof(int)) : 0,
                 o_reid = with_app ? take(N * PM * sizeof(int)) : 0;
    unsigned char* grown = nullptr;
    dev_alloc((void**)&grown, at);
    dev_free(img_dev);
    img_dev = grown, img_cap = (int)N;
    off_dist = o_dist, off_np = o_np, off_ppl = o_ppl, off_ids = o_ids, off_place = o_place;
    off_smooth = o_smooth, off_src = o_src, off_cand = o_cand, img_smooth = with;
    off_desc = o_desc, off_qdesc = o_qdesc, off_reid = o_reid, img_appear = with_app;
  }
}

void Tracker::enqueue(int nb, int P, const int* slot_of, const int* d_np, const double* d_ppl, long long* ids, int* place, double* dist,
                      void* stream, const SmoothOut* so, const BeforeDone* before_done, const int* d_cand, const int* d_desc, int* reid) {
  hipStream_t s = (hipStream_t)stream;
  long long* d_ids = (long long*)(img_dev + off_ids);
  int* d_place = (int*)(img_dev + off_place);
  double* d_dist = (double*)(img_dev + off_dist);
  TrackSlotMap map{};
  for (int b = 0; b < nb; ++b) track_slot_map_set(map, b, slot_of ? slot_of[b] : b);
  HIPCHECK(hipStreamWaitEvent(s, (hipEvent_t)done, 0));
  TrackSmooth sm{};
  const bool on = smooth.enabled != 0;
  if (on) {
    sm.min_cutoff = smooth.min_cutoff, sm.beta = smooth.beta, sm.d_cutoff = smooth.d_cutoff, sm.max_hold = smooth.max_hold;
    sm.filt = (TrackFilter*)filt_dev;
    sm.smooth = (double*)(img_dev + off_smooth), sm.src = (int*)(img_dev + off_src);
    if (so && so->d_cand) sm.cand_in = so->d_cand, sm.cand_out = (int*)(img_dev + off_cand);
  }
  TrackAppear ap{};
  const bool app = appear.enabled != 0;
  if (app) {
    ap.min_pixels = appear.min_pixels, ap.alpha256 = appear.alpha256, ap.reid_max = appear.reid_max, ap.max_age = appear.max_age;
    ap.min_hits = appear.min_hits, ap.state = app_dev, ap.slot_stride = app_stride;
    ap.desc = d_desc, ap.qdesc = (int*)(img_dev + off_qdesc), ap.reid = (int*)(img_dev + off_reid);
  }
  KCHECK(launch_track(slots, nb, P, tp, (const double*)(dev + off_sig), dev, slot_stride, d_dist, d_np, d_ppl, d_ids, d_place, map, stream,
                      on ? &sm : nullptr, app ? &ap : nullptr));
  if (app && reid) HIPCHECK(hipMemcpyAsync(reid, ap.reid, (size_t)nb * P * sizeof(int), hipMemcpyDeviceToHost, s));
  if (on && so) {  // out of the shared scratch, in front of the event: the next update's launch waits for it
    const size_t e = (size_t)nb * P * tp.J;
    if (so->people) HIPCHECK(hipMemcpyAsync(so->people, sm.smooth, e * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (so->src) HIPCHECK(hipMemcpyAsync(so->src, sm.src, e * sizeof(int), hipMemcpyDeviceToHost, s));
    if (so->cand && sm.cand_out) HIPCHECK(hipMemcpyAsync(so->cand, sm.cand_out, e * sizeof(int), hipMemcpyDeviceToHost, s));
  }
  if (before_done && *before_done) (*before_done)(on ? sm.smooth : d_ppl, on ? sm.cand_out : d_cand, d_ids);  // likewise
  if (ids) HIPCHECK(hipMemcpyAsync(ids, d_ids, (size_t)nb * P * sizeof(long long), hipMemcpyDeviceToHost, s));
  if (place) HIPCHECK(hipMemcpyAsync(place, d_place, (size_t)nb * P * sizeof(int), hipMemcpyDeviceToHost, s));
  for (int b = 0; dist && b < nb; ++b)
    HIPCHECK(hipMemcpyAsync(dist + (size_t)b * tp.T * P, d_dist + (size_t)b * tp.T * kPeopleMaxPeople, (size_t)tp.T * P * sizeof(double),
                            hipMemcpyDeviceToHost, s));
  HIPCHECK(hipEventRecord((hipEvent_t)done, s));
}

bool Tracker::enqueue_chained(int nb, int P, const int* slot_of, const int* d_np, const double* d_ppl, const int* d_cand, long long* ids,
                              int* place, double* people, int* cand, void* stream, const BeforeDone* before_done) {
  if (!smooth.enabled) {
    enqueue(nb, P, slot_of, d_np, d_ppl, ids, place, nullptr, stream, nullptr, before_done, cand ? d_cand : nullptr);
    return false;
  }
  SmoothOut so;
  so.people = people, so.d_cand = cand ? d_cand : nullptr, so.cand = cand;
  enqueue(nb, P, slot_of, d_np, d_ppl, ids, place, nullptr, stream, &so, before_done);
  return true;
}

void Tracker::update(int nb, int P, const int* slot_of, const int* n_people, const double* people, long long* ids, int* place, double* dist,
                     double* smooth_out, int* src, bool smoothed, bool with_appearance, const int* desc, int* reid) {
  check_call("tracker_update", nb, P, tp.J, slot_of);
  if (with_appearance && !appear.enabled)
    bad("tracker_update_appearance", "appearance is off (dc_tracker_set_appearance): there is nothing to re-identify with");
  if (with_appearance && (smooth_out || src) && !smooth.enabled)
    bad("tracker_update_appearance", "smoothing is off (dc_tracker_set_smoothing): smooth and src must be NULL");
  if (smoothed && !smooth.enabled)
    bad("tracker_update_smoothed", "smoothing is off (dc_tracker_set_smoothing): there are no smoothed poses to return");
  for (int b = 0; b < nb; ++b)
    if (n_people[b] < 0 || n_people[b] > P)
      bad("tracker_update", "n_people[" + std::to_string(b) + "] = " + std::to_string(n_people[b]) + " is outside [0, P = " + std::to_string(P) + "]");
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "tracker_update() in CPU mode");
  if (device_count() <= 0) throw DcError(DC_EDEVICE, "no HIP device visible");
  const int d = Context::get().device;
  HIPCHECK(hipSetDevice(d));
  RuntimeLock rl;
  hipStream_t s = util_stream();
  prepare(d, nb, s);  // binds, allocates and zeroes, or DC_EDEVICE
  wait_done();        // the staging below is the tracker's own: an update still in flight reads it
  int* d_np = (int*)(img_dev + off_np);
  double* d_ppl = (double*)(img_dev + off_ppl);
  const size_t img = (size_t)P * tp.J * 3;
  HIPCHECK(hipMemcpyAsync(d_np, n_people, (size_t)nb * sizeof(int), hipMemcpyHostToDevice, s));
  // only the people that exist are read on either side
  for (int b = 0; b < nb; ++b)
    if (n_people[b] > 0)
      HIPCHECK(hipMemcpyAsync(d_ppl + (size_t)b * img, people + (size_t)b * img, (size_t)n_people[b] * tp.J * 3 * sizeof(double),
                              hipMemcpyHostToDevice, s));
  int* d_desc = nullptr;
  if (appear.enabled && desc) {  // whole: the kernel reads the people that exist only
    d_desc = (int*)(img_dev + off_desc);
    HIPCHECK(hipMemcpyAsync(d_desc, desc, (size_t)nb * P * kTrackModel * sizeof(int), hipMemcpyHostToDevice, s));
  }
  SmoothOut so;
  so.people = smooth_out, so.src = src;
  enqueue(nb, P, slot_of, d_np, d_ppl, ids, place, dist, s, &so, nullptr, nullptr, d_desc, reid);
  HIPCHECK(hipStreamSynchronize(s));
}

void Tracker::reset(int slot) {
  if (slot < -1 || slot >= slots) bad("tracker_reset", "slot must be in [0, " + std::to_string(slots) + ") or -1 for all");
  if (!dev) return;  // nothing has been tracked yet
  RuntimeLock rl;
  DeviceScope on(device);
  wait_done();
  hipStream_t s = util_stream();
  if (slot < 0) HIPCHECK(hipMemsetAsync(dev, 0, (size_t)slots * slot_stride, s));
  else HIPCHECK(hipMemsetAsync(dev + (size_t)slot * slot_stride, 0, slot_stride, s));
  if (filt_dev) {  // the slot's filters go with its tracks
    const size_t per = (size_t)tp.T * tp.J * sizeof(TrackFilter);
    if (slot < 0) HIPCHECK(hipMemsetAsync(filt_dev, 0, (size_t)slots * per, s));
    else HIPCHECK(hipMemsetAsync(filt_dev + (size_t)slot * per, 0, per, s));
  }
  if (app_dev) {  // ... and its models and gallery
    if (slot < 0) HIPCHECK(hipMemsetAsync(app_dev, 0, (size_t)slots * app_stride, s));
    else HIPCHECK(hipMemsetAsync(app_dev + (size_t)slot * app_stride, 0, app_stride, s));
  }
  HIPCHECK(hipStreamSynchronize(s));
}

void Tracker::set_appearance(const dc_track_appearance_params* p) {
  const std::string who = "tracker_set_appearance";
  AppearParams q;
  if (p && p->enabled) {
    if (p->enabled != 1) bad(who, "enabled must be 0 or 1");
    if (p->min_pixels < 1) bad(who, "min_pixels must be >= 1");
    if (p->alpha256 < 0 || p->alpha256 > 256) bad(who, "alpha256 must be in [0, 256]");
    if (p->reid_max < 0 || p->reid_max > 3 * 4096) bad(who, "reid_max must be in [0, 12288]");
    if (p->max_age < 0 || p->max_age > 100000) bad(who, "max_age must be in [0, 100000]");
    if (p->min_hits < 1) bad(who, "min_hits must be >= 1");
    q.enabled = 1, q.min_pixels = p->min_pixels, q.alpha256 = p->alpha256, q.reid_max = p->reid_max, q.max_age = p->max_age;
    q.min_hits = p->min_hits;
  }
  RuntimeLock rl;  // no update is being enqueued meanwhile
  if (dev) {
    DeviceScope on(device);
    wait_done();
  }
  if (q.enabled && !appear.enabled) app_clear = true;  // off -> on: the next update starts with empty models and galleries
  appear = q;
}

void Tracker::appearance_state(int slot, int* track_model, int* track_valid, long long* gallery_ids, int* gallery_age, int* gallery_model) {
  if (slot < 0 || slot >= slots) bad("tracker_appearance_state", "slot must be in [0, " + std::to_string(slots) + ")");
  const int T = tp.T;
  std::vector<unsigned char> block(track_appear_bytes(T), 0), tracks(track_slot_bytes(T, tp.J), 0);  // all zero: nothing valid, empty gallery
  if (dev && app_dev && appear.enabled && !app_clear) {
    RuntimeLock rl;
    DeviceScope on(device);
    wait_done();
    hipStream_t s = util_stream();
    HIPCHECK(hipMemcpyAsync(block.data(), app_dev + (size_t)slot * app_stride, block.size(), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(tracks.data(), dev + (size_t)slot * slot_stride, tracks.size(), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  const TrackAppearSlot as = track_appear_slot(block.data(), T);
  const TrackSlot st = track_slot(tracks.data(), T, tp.J);
  for (int i = 0; i < T; ++i) {  // a free place keeps stale values on the device: it reports none
    const bool has = st.live[i] != 0 && as.valid[i] != 0;
    if (track_valid) track_valid[i] = has ? 1 : 0;
    for (int k = 0; track_model && k < kTrackModel; ++k) track_model[(size_t)i * kTrackModel + k] = has ? as.model[(size_t)i * kTrackModel + k] : 0;
  }
  for (int g = 0; g < kTrackGallery; ++g) {
    const bool occ = as.gocc[g] != 0;
    if (gallery_ids) gallery_ids[g] = occ ? as.gid[g] : -1;
    if (gallery_age) gallery_age[g] = occ ? as.gage[g] : -1;
    for (int k = 0; gallery_model && k < kTrackModel; ++k) gallery_model[(size_t)g * kTrackModel + k] = occ ? as.gmodel[(size_t)g * kTrackModel + k] : 0;
  }
}

void Tracker::set_smoothing(const dc_track_smooth_params* p) {
  const std::string who = "tracker_set_smoothing";
  SmoothParams q;
  if (p && p->enabled) {
    if (p->enabled != 1) bad(who, "enabled must be 0 or 1");
    if (!(std::isfinite(p->min_cutoff) && p->min_cutoff > 0)) bad(who, "min_cutoff must be finite and > 0");
    if (!(std::isfinite(p->beta) && p->beta >= 0)) bad(who, "beta must be finite and >= 0");
    if (!(std::isfinite(p->d_cutoff) && p->d_cutoff > 0)) bad(who, "d_cutoff must be finite and > 0");
    if (p->max_hold < 0 || p->max_hold > 1000) bad(who, "max_hold must be in [0, 1000]");
    q.enabled = 1, q.min_cutoff = p->min_cutoff, q.beta = p->beta, q.d_cutoff = p->d_cutoff, q.max_hold = p->max_hold;
  }
  RuntimeLock rl;  // no update is being enqueued meanwhile
  if (dev) {
    DeviceScope on(device);
    wait_done();
  }
  if (q.enabled && !smooth.enabled) filt_clear = true;  // off -> on: the next update starts with empty filters
  smooth = q;
}

void Tracker::smooth_state(int slot, double* poses, int* gap) {
  if (slot < 0 || slot >= slots) bad("tracker_smooth_state", "slot must be in [0, " + std::to_string(slots) + ")");
  const size_t n = (size_t)tp.T * tp.J;
  std::vector<TrackFilter> f(n);  // value-initialised: every filter empty
  if (filt_dev && smooth.enabled && !filt_clear) {
    RuntimeLock rl;
    DeviceScope on(device);
    wait_done();
    hipStream_t s = util_stream();
    HIPCHECK(hipMemcpyAsync(f.data(), filt_dev + (size_t)slot * n * sizeof(TrackFilter), n * sizeof(TrackFilter), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  for (size_t e = 0; e < n; ++e) {
    const TrackFilter& g = f[e];
    const bool has = g.n > 0;
    if (poses) {
      poses[e * 3] = has ? g.fx + g.dx * (double)g.gap : 0.0;
      poses[e * 3 + 1] = has ? g.fy + g.dy * (double)g.gap : 0.0;
      poses[e * 3 + 2] = has ? g.fs : 0.0;
    }
    if (gap) gap[e] = has ? g.gap : -1;
  }
}

void Tracker::set_option(int key, int value) {
  if (key != DC_TRACK_OPT_ASSIGN) bad("tracker_set_option", "unknown key " + std::to_string(key));
  if (value != DC_TRACK_ASSIGN_GREEDY && value != DC_TRACK_ASSIGN_OPTIMAL)
    bad("tracker_set_option", "DC_TRACK_OPT_ASSIGN takes DC_TRACK_ASSIGN_GREEDY (0) or DC_TRACK_ASSIGN_OPTIMAL (1), not value " + std::to_string(value));
  RuntimeLock rl;  // no update is being enqueued meanwhile
  if (dev) {       // nothing has been tracked yet otherwise, and nothing is in flight
    DeviceScope on(device);
    wait_done();
  }
  tp.assign = value;
}

int Tracker::get_option(int key) const {
  if (key != DC_TRACK_OPT_ASSIGN) bad("tracker_get_option", "unknown key " + std::to_string(key));
  return tp.assign;
}

void Tracker::state(int slot, long long* ids, int* misses, int* hits, double* poses) {
  if (slot < 0 || slot >= slots) bad("tracker_state", "slot must be in [0, " + std::to_string(slots) + ")");
  const int T = tp.T, J = tp.J;
  std::vector<unsigned char> block(track_slot_bytes(T, J), 0);  // all zero: every place free
  if (dev) {
    RuntimeLock rl;
    DeviceScope on(device);
    wait_done();
    hipStream_t s = util_stream();
    HIPCHECK(hipMemcpyAsync(block.data(), dev + (size_t)slot * slot_stride, block.size(), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  const TrackSlot st = track_slot(block.data(), T, J);
  for (int i = 0; i < T; ++i) {
    const bool lv = st.live[i] != 0;
    if (ids) ids[i] = lv ? st.id[i] : -1;
    if (misses) misses[i] = lv ? st.misses[i] : 0;
    if (hits) hits[i] = lv ? st.hits[i] : 0;
    for (int k = 0; poses && k < J * 3; ++k) poses[(size_t)i * J * 3 + k] = lv ? st.pose[(size_t)i * J * 3 + k] : 0.0;
  }
}

}  // namespace dc
