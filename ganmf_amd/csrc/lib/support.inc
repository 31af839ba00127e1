// support.inc -- profile scopes, tensor allocation, reference-variable views of the folded tensors
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

struct Scope {
  ganmf_handle* h;
  bool on;
  ProfRec r;
  hipStream_t s;
  Scope(ganmf_handle* h_, int tag, double flops, double bytes, hipStream_t st = nullptr)
      : h(h_), on(h_->prof), s(st ? st : h_->st) {
    if (on) {
      r.tag = tag; r.flops = flops; r.bytes = bytes;
      hipEventCreate(&r.a); hipEventCreate(&r.b);
      hipEventRecord(r.a, s);
      launch_prof() = LaunchProf{r.a, r.b, 0};      // the first kernel launched inside the scope stamps both events itself
    }
  }
  ~Scope() {
    if (on) {
      // exactly one kernel: its own start / end are on the events.  None (a collective) or several: bracket as before.
      if (launch_prof().count != 1) hipEventRecord(r.b, s);
      launch_prof() = LaunchProf{};
      h->recs.push_back(r);
    }
  }
};

int alloc_tensor(Tensor& t, int rows, int cols, bool grad_separate, int world, int ld = 0) {
  t.rows = rows; t.cols = cols; t.ld = ld ? ld : round_up(cols + 1, LD_ALIGN);
  // data-parallel runs reduce-scatter the gradient, update one slice per rank and all-gather the parameter: every
  // buffer holds world equal slices (the tail past padded() is zero and stays zero: Adam's fixed point)
  const size_t w = (size_t)std::max(world, 1);
  t.cap = ((t.padded() + w - 1) / w + 63) / 64 * 64 * w;
  TRY(t.p.alloc(t.cap, true));
  TRY(t.m.alloc(t.cap, true));
  TRY(t.v.alloc(t.cap, true));
  TRY(t.best.alloc(t.cap, true));
  if (grad_separate) { TRY(t.g_own.alloc(t.cap, true)); t.g = t.g_own; }
  return 0;
}

// GANMF_MODEL_ITEMSIM holds the weighted URM and an item similarity matrix, no tensor at all: the entries that read or write factors,
// discriminator weights or their snapshots refuse such a handle before they touch anything
int needs_tensors(const ganmf_handle* h, const char* who) {
  if (h->cfg.model == GANMF_MODEL_ITEMSIM)
    return fail(-1, "%s: a GANMF_MODEL_ITEMSIM handle holds a weighted URM and an item similarity matrix and has no tensors", who);
  return 0;
}

// GANMF_MODEL_CFGAN holds two MLPs and no factor tensors, trains through ganmf_cfgan_* and scores through its generator: the entries
// built on factors or on the other models' steps refuse it before they touch anything
int not_cfgan(const ganmf_handle* h, const char* who) {
  if (h->cfg.model == GANMF_MODEL_CFGAN)
    return fail(-1, "%s: not defined on a GANMF_MODEL_CFGAN handle (two MLPs, no factor tensors; it trains through ganmf_cfgan_* and scores through its generator)", who);
  if (h->cfg.model == GANMF_MODEL_CAAE)      // the same entries refuse CAAE: its factor tensors are a discriminator's, trained through ganmf_caae_*
    return fail(-1, "%s: not defined on a GANMF_MODEL_CAAE handle (a pairwise discriminator and two MLP generators; it trains through ganmf_caae_* and scores through its generator G)", who);
  return 0;
}

// the gate of the ganmf_cfgan_* / ganmf_caae_* entries behind their _init: a handle of `model`, initialised, with a URM where needed
int model_ready(ganmf_handle* h, const char* who, int model, bool need_urm) {
  const bool cfgan = model == GANMF_MODEL_CFGAN;
  if (!h) return fail(-1, "%s: null handle", who);
  if (h->cfg.model != model) return fail(-1, "%s: needs a GANMF_MODEL_%s handle", who, cfgan ? "CFGAN" : "CAAE");
  if (!(cfgan ? h->cf.ready : h->ca.ready))
    return fail(-1, "%s: ganmf_%s_init has not been called on this handle", who, cfgan ? "cfgan" : "caae");
  if (need_urm && !h->has_urm) return fail(-1, "%s: ganmf_set_urm_csr has not been called", who);
  return 0;
}

// A reference variable as up to two row segments of a folded tensor.
struct Seg { Tensor* t; int row0, col0, rows, cols, host_row0; };
struct View { int rows, cols, nseg; Seg seg[2]; };

bool find_view(ganmf_handle* h, int id, View* v) {
  auto one = [&](Tensor* t, int row0, int col0, int rows, int cols) {
    v->rows = rows; v->cols = cols; v->nseg = 1; v->seg[0] = {t, row0, col0, rows, cols, 0};
    return true;
  };
  if (h->cfg.model == GANMF_MODEL_CFGAN) {
    // discriminator ids as DisGANMF's (layer 0 is [2N, e]: condition rows then input rows, the bias is row 2N of the folded tensor);
    // generator ids from GANMF_T_CFGAN_G0, laid out the same way (G_output/kernel [g, N], G_output/bias [N])
    const int N = h->N, e = h->e, g = h->cf.gen.g, L = h->L, Lg = h->cf.gen.Lg;
    if (id >= 0 && id <= 2 * L + 1) {
      if (id == 2 * L) { v->rows = e; v->cols = 1; v->nseg = 1; v->seg[0] = {&h->Wo, 0, 0, 1, e, 0}; return true; }
      if (id == 2 * L + 1) return one(&h->Wo, 0, e, 1, 1);
      const int l = id / 2;
      if (id & 1) return one(&h->Wl[l], l == 0 ? 2 * N : e, 0, 1, e);
      return one(&h->Wl[l], 0, 0, l == 0 ? 2 * N : e, e);
    }
    const int gid = id - GANMF_T_CFGAN_G0;
    if (!h->cf.ready || gid < 0 || gid > 2 * Lg + 1) return false;
    if (gid == 2 * Lg) return one(&h->cf.gen.Go, 0, 0, g, N);
    if (gid == 2 * Lg + 1) return one(&h->cf.gen.Go, g, 0, 1, N);
    const int l = gid / 2;
    if (gid & 1) return one(&h->cf.gen.Gl[l], l == 0 ? N : g, 0, 1, g);
    return one(&h->cf.gen.Gl[l], 0, 0, l == 0 ? N : g, g);
  }
  if (h->cfg.model == GANMF_MODEL_CAAE) {
    // D: disc_user_embeddings / disc_item_embeddings under the factor ids, disc_item_bias [1, N]; G from GANMF_T_CAAE_G0 and G' from
    // GANMF_T_CAAE_GPR0, each laid out as CFGAN's generator (2l g_layer_l/kernel, 2l+1 its bias, 2Lg reconstruction/kernel, 2Lg+1 its bias)
    if (id == GANMF_T_USER_EMB) return one(&h->Ue, 0, 0, h->U, h->k);
    if (id == GANMF_T_ITEM_EMB) return one(&h->V, 0, 0, h->N, h->k);
    if (!h->ca.ready) return false;
    if (id == GANMF_T_CAAE_ITEM_BIAS) return one(&h->ca.bias, 0, 0, 1, h->N);
    const int which = id >= GANMF_T_CAAE_GPR0 ? 1 : 0;
    const int gid = id - (which ? GANMF_T_CAAE_GPR0 : GANMF_T_CAAE_G0);
    ProfileMlp& gn = h->ca.gen[which];
    const int N = h->N, g = gn.g, Lg = gn.Lg;
    if (gid < 0 || gid > 2 * Lg + 1) return false;
    if (gid == 2 * Lg) return one(&gn.Go, 0, 0, g, N);
    if (gid == 2 * Lg + 1) return one(&gn.Go, g, 0, 1, N);
    const int l = gid / 2;
    if (gid & 1) return one(&gn.Gl[l], l == 0 ? N : g, 0, 1, g);
    return one(&gn.Gl[l], 0, 0, l == 0 ? N : g, g);
  }
  if (id == GANMF_T_USER_EMB) return one(&h->Ue, 0, 0, h->U, h->k);
  if (id == GANMF_T_ITEM_EMB) return one(&h->V, 0, 0, h->N, h->k);
  if (h->cfg.model == GANMF_MODEL_MF) return false;      // the two factor tensors are all such a handle holds
  if (h->cfg.model == GANMF_MODEL_GANMF) {
    switch (id) {
      case 0: return one(&h->We, 0, 0, h->N, h->e);      // autoencoder/encoding/kernel
      case 1: return one(&h->We, h->N, 0, 1, h->e);      // autoencoder/encoding/bias  (row N of We_ext)
      case 2: return one(&h->Wd, 0, 0, h->e, h->N);      // autoencoder/decoding/kernel
      case 3: return one(&h->Wd, h->e, 0, 1, h->N);      // autoencoder/decoding/bias  (row e of Wd_ext)
      default: return false;
    }
  }
  // DisGANMF: 2l layer_l/kernel, 2l+1 layer_l/bias, 2L D_output/kernel [e,1], 2L+1 D_output/bias [1]
  if (id < 0 || id > 2 * h->L + 1) return false;
  if (id == 2 * h->L) { v->rows = h->e; v->cols = 1; v->nseg = 1; v->seg[0] = {&h->Wo, 0, 0, 1, h->e, 0}; return true; }
  if (id == 2 * h->L + 1) return one(&h->Wo, 0, h->e, 1, 1);
  const int l = id / 2;
  Tensor* t = &h->Wl[l];
  if (id & 1) return one(t, l == 0 ? h->N : h->e, 0, 1, h->e);
  if (l > 0) return one(t, 0, 0, h->e, h->e);
  // layer_0/kernel is [N+1, e] in the reference with row 0 multiplying float(uid) (DisGANMF.py:59)
  v->rows = h->N + 1; v->cols = h->e; v->nseg = 2;
  v->seg[0] = {t, h->N + 1, 0, 1, h->e, 0};
  v->seg[1] = {t, 0, 0, h->N, h->e, 1};
  return true;
}

std::vector<Tensor*> all_tensors(ganmf_handle* h) {
  std::vector<Tensor*> v;
  if (h->cfg.model == GANMF_MODEL_ITEMSIM) return v;
  if (h->cfg.model == GANMF_MODEL_CFGAN) {      // no factor tensors: the discriminator's layers, then the generator's
    for (auto& t : h->Wl) v.push_back(&t);
    v.push_back(&h->Wo);
    if (h->cf.ready) for (Tensor* t : h->cf.gen.tensors()) v.push_back(t);
    return v;
  }
  v = {&h->Ue, &h->V};
  if (h->cfg.model == GANMF_MODEL_CAAE && h->ca.ready) {      // P, Q, then b and the layers of G and G'
    v.push_back(&h->ca.bias);
    for (ProfileMlp& gn : h->ca.gen) for (Tensor* t : gn.tensors()) v.push_back(t);
  }
  if (h->cfg.model == GANMF_MODEL_GANMF) { v.push_back(&h->We); v.push_back(&h->Wd); }
  else if (h->cfg.model == GANMF_MODEL_DISGANMF) { for (auto& t : h->Wl) v.push_back(&t); v.push_back(&h->Wo); }
  return v;
}

float* slot_ptr(Tensor* t, int slot) {
  switch (slot) {
    case GANMF_SLOT_PARAM: return t->p;
    case GANMF_SLOT_ADAM_M: return t->m;
    case GANMF_SLOT_ADAM_V: return t->v;
    case GANMF_SLOT_BEST: return t->best;
    default: return nullptr;
  }
}

// MFMA_F16: power of two that brings an operand carrying the loss gradient's 1/(B.N) (GANMF: mean over B.N reconstruction
// errors) or 1/B (DisGANMF: mean over B cross-entropies, times an output weight of ~2^-5) into fp16's normal range
inline float grad_scale(const ganmf_handle* h, int b_global) {
  if (h->tune.mode != MFMA_F16) return 0.f;
  const float lg = h->cfg.model == GANMF_MODEL_GANMF ? log2f((float)b_global * (float)h->N) : log2f((float)b_global) + 6.f;
  return exp2f(roundf(lg));
}
inline bool low_precision(const ganmf_handle* h) { return h->tune.mode == MFMA_F16 || h->tune.mode == MFMA_BF16; }

inline double gemm_flops(double M, double N, double K) { return 2.0 * M * N * K; }
inline double gemm_bytes(double M, double N, double K) { return 4.0 * (M * K + N * K + M * N); }

