// sparse_pairwise.cpp — DC_OPT_SPARSE_PAIRWISE: the pairwise head of a net that leaves `next_pred` out of its plan, evaluated at the
// cells its consumers read (dc_net_assemble_people, dc_net_decode_pairwise, dc_net_pairwise_at).  The rule: include/deepcut_hip.h,
// dc_net_pairwise_at; the kernels: sparse_head.hip.  NetGroup is out of scope: its members keep refusing without `next_pred`.
#include "net_internal.h"

namespace dc {

// The pairwise head, from the layer list alone (the lowering's head ops are dead when `next_pred` is left out): `next_pred` is the top of
// an Eltwise SUM of a 1x1 / stride 1 / pad 0 Convolution and the Crop of a kernel 3 / stride 2 / pad 0 / dilation 1 / group 1
// Deconvolution.  Anything else is DC_EUNSUP naming the layer.
Net::PairHead Net::find_pair_head() const {
  auto it = blob_index.find("next_pred");
  if (it == blob_index.end()) throw DcError(DC_EUNSUP, "DC_OPT_SPARSE_PAIRWISE: the net has no 'next_pred' blob");
  auto sid = [&](int blob) { return blobs[blob]->st->id; };
  // the layer that last wrote a storage before layer `before` (splits share their bottom's storage and write nothing)
  auto producer = [&](int storage, int before) {
    for (int i = before - 1; i >= 0; --i) {
      if (layers[i].is_split) continue;
      for (int tb : layers[i].tops)
        if (sid(tb) == storage) return i;
    }
    return -1;
  };
  auto unsup = [](const LayerRec& L, const std::string& why) {
    throw DcError(DC_EUNSUP, "DC_OPT_SPARSE_PAIRWISE: layer '" + L.name + "' (" + L.type + ") " + why);
  };
  PairHead h;
  h.elt = producer(sid(it->second), (int)layers.size());
  if (h.elt < 0) throw DcError(DC_EUNSUP, "DC_OPT_SPARSE_PAIRWISE: 'next_pred' is not the top of a layer");
  const LayerRec& E = layers[h.elt];
  if (E.type != "Eltwise" || E.bottoms.size() != 2) unsup(E, "writes next_pred: the pairwise head must end in an Eltwise SUM of two bottoms");
  for (int bi = 0; bi < 2; ++bi) {
    const int pl = producer(sid(E.bottoms[bi]), h.elt);
    if (pl < 0) unsup(E, "has a bottom that no layer writes");
    const LayerRec& P = layers[pl];
    if (P.type == "Convolution") {
      if (h.conv >= 0) unsup(P, "is the head's second Convolution: one bottom must be the Crop of a Deconvolution");
      const ConvSpec& c = P.conv;
      if (c.kh != 1 || c.kw != 1 || c.sh != 1 || c.sw != 1 || c.ph != 0 || c.pw != 0 || c.group != 1)
        unsup(P, "must be a 1x1 convolution with stride 1, pad 0, group 1");
      h.conv = pl;
    } else if (P.type == "Crop") {
      if (h.crop >= 0) unsup(P, "is the head's second Crop: one bottom must be a 1x1 Convolution");
      h.crop = pl;
      const int dl = producer(sid(P.bottoms[0]), pl);
      if (dl < 0 || layers[dl].type != "Deconvolution") unsup(dl < 0 ? P : layers[dl], "feeds the head's Crop: a Deconvolution is needed there");
      const ConvSpec& c = layers[dl].conv;
      if (c.kh != 3 || c.kw != 3 || c.sh != 2 || c.sw != 2 || c.ph != 0 || c.pw != 0 || c.dh != 1 || c.dw != 1 || c.group != 1)
        unsup(layers[dl], "must be a deconvolution with kernel 3, stride 2, pad 0, dilation 1, group 1");
      h.deconv = dl;
    } else {
      unsup(P, "feeds the head's Eltwise: a 1x1 Convolution and the Crop of a Deconvolution are needed there");
    }
  }
  if (h.conv < 0 || h.crop < 0) unsup(E, "needs one 1x1 Convolution and one Crop of a Deconvolution as bottoms");
  if (layers[h.conv].conv.num_output != layers[h.deconv].conv.num_output) unsup(E, "adds maps of different channel counts");
  return h;
}

void Net::set_sparse_pairwise(int v) {
  if (v != 0 && v != 1) throw DcError(DC_EINVAL, "DC_OPT_SPARSE_PAIRWISE must be 0 or 1");
  if (v) (void)find_pair_head();
  sparse_pairwise = v;
}

bool Net::next_in_plan() const {
  auto it = blob_index.find("next_pred");
  if (it == blob_index.end()) return false;
  const Storage& s = *blobs[it->second]->st;
  return !(s.elided && s.view_of < 0);
}

// The device image of a materialised activation, the way map_ref brings an output map (host-authoritative: uploaded first)
static void act_image(Net& n, Storage& s, const std::string& name, const void*& ptr, int& cp, int& c0, int& ek) {
  if (s.elided && s.view_of < 0)
    throw DcError(DC_EUNSUP, "DC_OPT_SPARSE_PAIRWISE: '" + name + "', an input of the pairwise head, is not materialised in the current plan");
  if (s.head == UNINITIALIZED) throw DcError(DC_EINVAL, "'" + name + "': run forward() first");
  if (s.shape.size() != 4) throw DcError(DC_ESHAPE, "'" + name + "' is not a 4-D map");
  if (s.view_of >= 0) {
    Storage& b = *n.storages[s.view_of];
    ptr = b.dev, cp = b.cp(), c0 = s.view_c0, ek = b.ekind;
  } else {
    if (s.head == HEAD_AT_CPU) n.sync_to_device(s);
    ptr = s.dev, cp = s.cp(), c0 = 0, ek = s.ekind;
  }
}

// Everything the two launches need: the inputs' device images, the packed filters (once per model and element type, in
// ModelShared::vec_by_key like every other filter image, dropped with weights_gen), and this net's scratch: the float32 map
// [NB][H][W][C], the class lists for `nslots` slots and room for `ntriples` (image, row, col) triples.
Net::SparseNext Net::sparse_next(int nslots, int ntriples) {
  const PairHead h = find_pair_head();
  check_weights();  // a parameter written since the last forward: the image below is packed from what the blobs hold now
  const LayerRec& CL = layers[h.conv];
  const LayerRec& DL = layers[h.deconv];
  const LayerRec& CR = layers[h.crop];
  Storage& X3 = *blobs[CL.bottoms[0]]->st;
  Storage& X5 = *blobs[DL.bottoms[0]]->st;
  Storage& NX = *blobs[blob_index.at("next_pred")]->st;
  if (NX.shape.size() != 4) throw DcError(DC_ESHAPE, "'next_pred' is not a 4-D map");
  SparseNext r{};
  SparseHeadArgs& a = r.a;
  int c03 = 0, c05 = 0, ek3 = 0, ek5 = 0;
  act_image(*this, X3, blobs[CL.bottoms[0]]->name, a.x3, a.cp3, c03, ek3);
  act_image(*this, X5, blobs[DL.bottoms[0]]->name, a.x5, a.cp5, c05, ek5);
  if (ek3 != ek5) throw DcError(DC_EUNSUP, "DC_OPT_SPARSE_PAIRWISE: the head's two inputs differ in element type");
  const int es = elem_kind_size(ek3);
  a.x3 = (const unsigned char*)a.x3 + (size_t)c03 * es;
  a.x5 = (const unsigned char*)a.x5 + (size_t)c05 * es;
  a.K3 = X3.dim(1), a.K5 = X5.dim(1), a.Cout = CL.conv.num_output;
  a.NB = NX.dim(0), a.H = NX.dim(2), a.W = NX.dim(3), a.h5 = X5.dim(2), a.w5 = X5.dim(3);
  a.oh = CR.crop_oh, a.ow = CR.crop_ow;
  if (NX.dim(1) != a.Cout || X3.dim(0) != a.NB || X5.dim(0) != a.NB || X3.dim(2) != a.H || X3.dim(3) != a.W || a.oh < 0 || a.ow < 0)
    throw DcError(DC_ESHAPE, "DC_OPT_SPARSE_PAIRWISE: the head's inputs do not have next_pred's batch and map size");
  a.vec3 = a.K3 % 4 == 0 && a.cp3 % 4 == 0 && c03 % 4 == 0;
  a.vec5 = a.K5 % 4 == 0 && a.cp5 % 4 == 0 && c05 % 4 == 0;

  // the filter image and the bias
  const std::string key = std::string("sparse_head:") + elem_kind_name(ek3) + ":" + std::to_string(h.elt);
  {
    std::lock_guard<std::mutex> lk(shared->mu);
    refresh_pack_cache();
    auto get = [&](const std::string& k, const std::function<void(std::vector<float>&)>& fill) {
      auto it = shared->vec_by_key.find(k);
      if (it != shared->vec_by_key.end()) return it->second;
      auto v = std::make_shared<DevVec>();
      fill(v->host);
      shared->vec_by_key[k] = v;
      return v;
    };
    sparse_w_ = get(key, [&](std::vector<float>& hv) {
      hv.resize(sparse_head_image_floats(a.Cout, a.K3, a.K5));
      sparse_head_pack_filters(CL.params[0]->st->host_ptr(), DL.params[0]->st->host_ptr(), a.Cout, a.K3, a.K5, hv.data());
      ++stats.sparse_packs;
    });
    sparse_b_ = get(key + ":bias", [&](std::vector<float>& hv) {
      hv.assign(a.Cout, 0.f);
      const float* bs = CL.conv.bias ? CL.params[1]->st->host_ptr() : nullptr;
      const float* bd = DL.conv.bias ? DL.params[1]->st->host_ptr() : nullptr;
      for (int c = 0; c < a.Cout; ++c) hv[c] = (bs ? bs[c] : 0.f) + (bd ? bd[c] : 0.f);
    });
    for (DevVec* v : {sparse_w_.get(), sparse_b_.get()}) {
      if (v->dev || v->host.empty()) continue;
      dev_alloc((void**)&v->dev, v->host.size() * sizeof(float));
      dev_upload(v->dev, v->host.data(), v->host.size() * sizeof(float), stream);
      if (v == sparse_w_.get()) KCHECK(launch_round_through(v->dev, (long)v->host.size(), ek3, stream));  // the filters as the dense head sees them
      HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
      v->uploaded = v->host.size();
      std::vector<float>().swap(v->host);  // the image lives in HBM only
    }
  }
  a.wimg = sparse_w_->dev, a.bias = sparse_b_->dev;

  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t map_b = up((size_t)a.NB * a.H * a.W * a.Cout * sizeof(float));
  const size_t work_b = up(((size_t)4 + 4 * (size_t)std::max(nslots, 1)) * sizeof(int));
  const size_t cell_b = up((size_t)std::max(ntriples, 1) * 3 * sizeof(int));
  if (map_b + work_b + cell_b > sparse_dev_.cap && stream) HIPCHECK(hipStreamSynchronize((hipStream_t)stream));  // before it is replaced
  unsigned char* base = (unsigned char*)sparse_dev_.get(map_b + work_b + cell_b);
  a.out = (float*)base;
  r.work = (int*)(base + map_b);
  r.cells = (int*)(base + map_b + work_b);
  r.ekind = ek3;
  r.N = MapRef{base, a.Cout, 0, 4, kElemF32, a.NB, a.Cout, a.H, a.W};
  return r;
}

// `next_pred` at the given cells of the last forward: a float32 map that holds the head at those cells and nothing defined elsewhere,
// the triples on the device beside it
Net::SparseNext Net::sparse_next_at(int ndet, const int* det) {
  SparseNext sn = sparse_next(ndet, ndet);
  HIPCHECK(hipMemcpyAsync(sn.cells, det, (size_t)ndet * 3 * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
  KCHECK(launch_sparse_head(sn.a, sn.ekind, nullptr, nullptr, 0, 0, sn.cells, ndet, sn.work, stream));
  return sn;
}

void Net::pairwise_at(int ndet, const int* det, float* out) {
  if (ndet < 0) throw DcError(DC_EINVAL, "pairwise_at: ndet >= 0");
  auto it = blob_index.find("next_pred");
  if (it == blob_index.end()) throw DcError(DC_EINVAL, "net has no 'next_pred' blob");
  const std::vector<int>& shp = blobs[it->second]->st->shape;
  if (shp.size() != 4) throw DcError(DC_ESHAPE, "'next_pred' is not a 4-D map");
  for (int d = 0; d < ndet; ++d)
    if (det[3 * d] < 0 || det[3 * d] >= shp[0] || det[3 * d + 1] < 0 || det[3 * d + 1] >= shp[2] || det[3 * d + 2] < 0 || det[3 * d + 2] >= shp[3])
      throw DcError(DC_EINVAL, "pairwise_at: detection " + std::to_string(d) + " (" + std::to_string(det[3 * d]) + ", " + std::to_string(det[3 * d + 1]) +
                                   ", " + std::to_string(det[3 * d + 2]) + ") is outside the " + std::to_string(shp[0]) + " maps of " +
                                   std::to_string(shp[2]) + " x " + std::to_string(shp[3]) + " cells");
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "pairwise_at() in CPU mode");
  const bool dense = next_in_plan();
  if (!dense && !sparse_pairwise) (void)map_ref("next_pred");  // DC_EUNSUP, in map_ref's words
  if (ndet == 0) return;
  ensure_device();
  MapRef N;
  const int* ddet;
  if (dense) {
    N = map_ref("next_pred");
    ddet = (const int*)scratch(((size_t)ndet * 3 * sizeof(int) + 255) / 256 * 256 + (size_t)ndet * N.C * sizeof(float));
    HIPCHECK(hipMemcpyAsync((void*)ddet, det, (size_t)ndet * 3 * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
  } else {
    const SparseNext sn = sparse_next_at(ndet, det);
    N = sn.N, ddet = sn.cells;
    (void)scratch(((size_t)ndet * 3 * sizeof(int) + 255) / 256 * 256 + (size_t)ndet * N.C * sizeof(float));
  }
  float* dout = (float*)(scratch_dev_.dev + ((size_t)ndet * 3 * sizeof(int) + 255) / 256 * 256);
  KCHECK(launch_map_gather(N.ptr, N.cp, N.c0, N.ek, N.H, N.W, N.C, ndet, ddet, dout, stream));
  HIPCHECK(hipMemcpyAsync(out, dout, (size_t)ndet * N.C * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
}

}  // namespace dc
