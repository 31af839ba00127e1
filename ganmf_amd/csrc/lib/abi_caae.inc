// abi_caae.inc -- C ABI: CAAE on a GANMF_MODEL_CAAE handle: ganmf_caae_init / _cdf / _draw_* / _get_draws / _d_step / _g_step / _epoch
// (caae_sample.hpp, caae_rows.hpp, step_caae.inc)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

int ganmf_caae_init(ganmf_handle* h, int32_t g_units, int32_t g_layers, int32_t d_bsize, int32_t m_batch, int32_t n_s, float lmbda,
                    float beta, float lr, uint64_t seed, const int32_t* k_rows) {
  const char* who = "ganmf_caae_init";
  if (!h || !k_rows) return fail(-1, "%s: null argument", who);
  if (h->cfg.model != GANMF_MODEL_CAAE) return fail(-1, "%s: needs a GANMF_MODEL_CAAE handle", who);
  if (h->ca.ready) return fail(-1, "%s: the handle is initialised already", who);
  if (g_units < 1 || g_layers < 1 || g_layers > 16) return fail(-1, "%s: needs g_units >= 1 and 1 <= g_layers <= 16", who);
  if (d_bsize < 1 || d_bsize > GANMF_CAAE_MAX_D_BSIZE) return fail(-1, "%s: needs 1 <= d_bsize <= %d", who, GANMF_CAAE_MAX_D_BSIZE);
  if (m_batch < 1 || m_batch > h->U) return fail(-1, "%s: m_batch %d: a batch of distinct users needs 1 <= m_batch <= %d", who, m_batch, h->U);
  if (n_s < 1 || n_s > (1 << 20)) return fail(-1, "%s: needs 1 <= n_s <= 2^20 policy draws per row", who);
  if (!std::isfinite(lmbda) || !std::isfinite(beta) || !std::isfinite(lr)) return fail(-1, "%s: lmbda, beta and lr must be finite", who);
  const int U = h->U, N = h->N;
  for (int u = 0; u < U; ++u)
    if (k_rows[u] < 0 || k_rows[u] > N) return fail(-1, "%s: k_rows[%d] = %d out of range [0,%d]", who, u, k_rows[u], N);
  HIP_TRY(hipSetDevice(h->dev));
  CaaeState& c = h->ca;
  c.d_bsize = d_bsize; c.Bm = m_batch; c.n_s = n_s; c.lmbda = lmbda; c.beta = beta; c.lr = lr; c.seed = seed;
  c.words = (N + 31) / 32;
  for (ProfileMlp& gn : c.gen) TRY(mlp_alloc(h, gn, g_units, g_layers, ACT_SIGMOID, ACT_SIGMOID, m_batch));
  TRY(alloc_tensor(c.bias, 1, N, false, 1));
  TRY(c.k_rows.alloc((size_t)U, true));
  HIP_TRY(hipMemcpy(c.k_rows, k_rows, (size_t)U * sizeof(int), hipMemcpyHostToDevice));
  TRY(c.cdf[0].alloc((size_t)U * h->ldN, true));
  TRY(c.cdf[1].alloc((size_t)U * h->ldN, true));
  TRY(c.lse_all.alloc((size_t)U, true));
  TRY(c.xt.alloc((size_t)3 * d_bsize, true));
  TRY(c.first.alloc((size_t)U + N, true));
  HIP_TRY(hipMemset(c.first, 0x7f, ((size_t)U + N) * sizeof(int)));
  HIP_TRY(hipDeviceSynchronize());
  TRY(c.xu.alloc((size_t)m_batch, true));
  TRY(c.xi.alloc((size_t)m_batch * n_s, true));
  TRY(c.xn.alloc((size_t)m_batch * c.words, true));
  TRY(c.Pg.alloc((size_t)d_bsize * h->ldk, true));
  TRY(c.Qi.alloc((size_t)d_bsize * h->ldk, true));
  TRY(c.Qj.alloc((size_t)d_bsize * h->ldk, true));
  TRY(c.coef.alloc((size_t)d_bsize, true));
  TRY(c.lt.alloc((size_t)d_bsize, true));
  TRY(c.rt.alloc((size_t)3 * d_bsize, true));      // rt, then the gathered biases [2 d_bsize]
  TRY(c.C.alloc((size_t)m_batch * h->ldN, true));
  TRY(c.R.alloc((size_t)m_batch * h->ldN, true));
  TRY(c.Rp.alloc((size_t)m_batch * h->ldN, true));
  TRY(c.cdfb.alloc((size_t)m_batch * h->ldN, true));
  TRY(c.dz.alloc((size_t)m_batch * h->ldN, true));
  TRY(c.dh0.alloc((size_t)m_batch * c.gen[0].ldg, true));
  TRY(c.dh1.alloc((size_t)m_batch * c.gen[0].ldg, true));
  TRY(c.lse.alloc((size_t)m_batch, true));
  TRY(c.reward.alloc((size_t)m_batch * n_s, true));
  TRY(c.la.alloc((size_t)m_batch, true));
  TRY(c.ae.alloc((size_t)m_batch, true));
  TRY(c.sq.alloc((size_t)(g_layers + 1) * CFGAN_SQ_BLOCKS, true));
  c.ready = true;
  ++h->param_version;
  return 0;
}

// the recorded draws' slots: `passes` discriminator passes and `steps` steps of either generator
static int caae_slots(ganmf_handle* h, int passes, int steps) {
  CaaeState& c = h->ca;
  const size_t nn = (size_t)std::max<long long>(h->urm.nnz, 1);
  TRY(c.neg.grow(h->st, (size_t)passes * 2 * nn, true));
  if (steps > c.step_slots) {
    HIP_TRY(hipStreamSynchronize(h->st));
    c.users.reset(); c.nu.reset(); c.items.reset();
    c.step_slots = 0;
    TRY(c.users.alloc((size_t)2 * steps * c.Bm, true));
    TRY(c.nu.alloc((size_t)steps * c.Bm * c.words, true));
    TRY(c.items.alloc((size_t)2 * steps * c.Bm * c.n_s, true));
    c.step_slots = steps;
  }
  return 0;
}
static int* caae_users_slot(CaaeState& c, int which, int step) { return c.users + ((size_t)which * c.step_slots + step) * c.Bm; }
static unsigned* caae_nu_slot(CaaeState& c, int step) { return c.nu + (size_t)step * c.Bm * c.words; }
static int* caae_items_slot(CaaeState& c, int which, int step) { return c.items + ((size_t)which * c.step_slots + step) * c.Bm * c.n_s; }

int ganmf_caae_cdf(ganmf_handle* h, int which, const int32_t* users, int32_t n, float* cdf_out, float* lse_out) {
  const char* who = "ganmf_caae_cdf";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, true));
  if (which != 0 && which != 1) return fail(-1, "%s: which must be 0 (G) or 1 (G')", who);
  CaaeState& c = h->ca;
  const int U = h->U, N = h->N;
  HIP_TRY(hipSetDevice(h->dev));
  if (!users) {      // all users into the resident array; rows [0, n) are downloaded when asked for
    if (n < 0 || n > U) return fail(-1, "%s: %d rows of %d", who, n, U);
    TRY(caae_cdf_all(h, which));
    HIP_TRY(hipStreamSynchronize(h->st));
    if (cdf_out && n) HIP_TRY(hipMemcpy2D(cdf_out, (size_t)N * 4, c.cdf[which], (size_t)h->ldN * 4, (size_t)N * 4, (size_t)n, hipMemcpyDeviceToHost));
    if (lse_out && n) HIP_TRY(hipMemcpy(lse_out, c.lse_all, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
  }
  if (n < 1 || n > c.Bm) return fail(-1, "%s: 1 to %d listed users per call, got %d", who, c.Bm, n);
  for (int i = 0; i < n; ++i)
    if (users[i] < 0 || users[i] >= U) return fail(-1, "%s: user %d out of range", who, users[i]);
  int* ud = c.xu;
  HIP_TRY(hipStreamSynchronize(h->st));
  HIP_TRY(hipMemcpy(ud, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  TRY(mlp_forward_rows(h, c.gen[which], ud, 0, n, c.R, h->ldN));
  GANMF_LAUNCH(caae_cdf_rows_kernel, dim3(n), dim3(256), 0, h->st, c.R.get(), h->ldN, N, c.cdfb.get(), h->ldN, c.lse.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->st));
  if (cdf_out) HIP_TRY(hipMemcpy2D(cdf_out, (size_t)N * 4, c.cdfb, (size_t)h->ldN * 4, (size_t)N * 4, (size_t)n, hipMemcpyDeviceToHost));
  if (lse_out) HIP_TRY(hipMemcpy(lse_out, c.lse, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_caae_draw_perm(ganmf_handle* h, int64_t epoch, int32_t* out) {
  const char* who = "ganmf_caae_draw_perm";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, true));
  if (epoch < 0) return fail(-1, "%s: negative epoch", who);
  HIP_TRY(hipSetDevice(h->dev));
  TRY(caae_draw_perm(h, epoch));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (out && h->urm.nnz) HIP_TRY(hipMemcpy(out, h->ca.perm, (size_t)h->urm.nnz * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_caae_draw_negatives(ganmf_handle* h, int64_t epoch, int32_t pass, int which, int32_t* out) {
  const char* who = "ganmf_caae_draw_negatives";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, true));
  if (epoch < 0 || pass < 0) return fail(-1, "%s: negative argument", who);
  if (which != 0 && which != 1) return fail(-1, "%s: which must be 0 (G) or 1 (G')", who);
  HIP_TRY(hipSetDevice(h->dev));
  TRY(caae_draw_perm(h, epoch));
  TRY(caae_slots(h, 1, 0));
  TRY(caae_draw_neg(h, epoch, pass, which, h->ca.neg));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (out && h->urm.nnz) HIP_TRY(hipMemcpy(out, h->ca.neg, (size_t)h->urm.nnz * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_caae_draw_batch(ganmf_handle* h, int64_t epoch, int which, int32_t step, int32_t* users, uint32_t* nu, int32_t* items,
                          float* cdf_out) {
  const char* who = "ganmf_caae_draw_batch";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, true));
  if (epoch < 0 || step < 0) return fail(-1, "%s: negative argument", who);
  if (which != 0 && which != 1) return fail(-1, "%s: which must be 0 (G) or 1 (G')", who);
  CaaeState& c = h->ca;
  HIP_TRY(hipSetDevice(h->dev));
  int* ud = c.xu;
  TRY(caae_draw_users(h, epoch, which, step, ud));
  if (which == 0) TRY(caae_draw_nu(h, epoch, step, ud, c.xn));
  TRY(caae_draw_items(h, epoch, which, step, ud, c.xi));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (users) HIP_TRY(hipMemcpy(users, ud, (size_t)c.Bm * sizeof(int), hipMemcpyDeviceToHost));
  if (nu && which == 0) HIP_TRY(hipMemcpy(nu, c.xn, (size_t)c.Bm * c.words * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (items) HIP_TRY(hipMemcpy(items, c.xi, (size_t)c.Bm * c.n_s * sizeof(int), hipMemcpyDeviceToHost));
  if (cdf_out) HIP_TRY(hipMemcpy2D(cdf_out, (size_t)h->N * 4, c.cdfb, (size_t)h->ldN * 4, (size_t)h->N * 4, (size_t)c.Bm, hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_caae_get_draws(ganmf_handle* h, int kind, int32_t index, void* out, int64_t bytes) {
  const char* who = "ganmf_caae_get_draws";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, false));
  if (!out) return fail(-1, "%s: null buffer", who);
  CaaeState& c = h->ca;
  const void* src = nullptr;
  size_t n = 0;
  const size_t nn = (size_t)c.rec_nnz;
  switch (kind) {
    case GANMF_CAAE_DRAW_PERM: src = c.perm; n = nn * 4; index = 0; break;
    case GANMF_CAAE_DRAW_CDF_G: case GANMF_CAAE_DRAW_CDF_GPR: {      // rows of the resident epoch-start CDF: one row per call
      const int q = kind - GANMF_CAAE_DRAW_CDF_G;
      if (index < 0 || index >= h->U) return fail(-1, "%s: row %d of %d", who, index, h->U);
      src = c.cdf[q] + (size_t)index * h->ldN; n = (size_t)h->N * 4; index = 0;
      break;
    }
    case GANMF_CAAE_DRAW_NEG_G: case GANMF_CAAE_DRAW_NEG_GPR:
      if (index < 0 || index >= c.rec_passes) return fail(-1, "%s: pass %d of %d recorded", who, index, c.rec_passes);
      src = c.neg + ((size_t)index * 2 + (kind - GANMF_CAAE_DRAW_NEG_G)) * std::max<size_t>(nn, 1); n = nn * 4;
      break;
    case GANMF_CAAE_DRAW_USERS_G: case GANMF_CAAE_DRAW_USERS_GPR: case GANMF_CAAE_DRAW_ITEMS_G: case GANMF_CAAE_DRAW_ITEMS_GPR: case GANMF_CAAE_DRAW_NU: {
      const int q = (kind == GANMF_CAAE_DRAW_USERS_GPR || kind == GANMF_CAAE_DRAW_ITEMS_GPR) ? 1 : 0;
      if (index < 0 || index >= c.rec_steps[q]) return fail(-1, "%s: step %d of %d recorded", who, index, c.rec_steps[q]);
      if (kind == GANMF_CAAE_DRAW_NU) { src = caae_nu_slot(c, index); n = (size_t)c.Bm * c.words * 4; }
      else if (kind == GANMF_CAAE_DRAW_USERS_G || kind == GANMF_CAAE_DRAW_USERS_GPR) { src = caae_users_slot(c, q, index); n = (size_t)c.Bm * 4; }
      else { src = caae_items_slot(c, q, index); n = (size_t)c.Bm * c.n_s * 4; }
      break;
    }
    default: return fail(-1, "%s: unknown kind %d", who, kind);
  }
  if ((int64_t)n != bytes) return fail(-1, "%s: kind %d holds %lld bytes, the buffer has %lld", who, kind, (long long)n, (long long)bytes);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (n) HIP_TRY(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_caae_d_step(ganmf_handle* h, const int32_t* users, const int32_t* pos_items, const int32_t* neg_items, int32_t count, float* loss) {
  const char* who = "ganmf_caae_d_step";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, false));
  if (!users || !pos_items || !neg_items) return fail(-1, "%s: null argument", who);
  CaaeState& c = h->ca;
  if (count < 1 || count > c.d_bsize) return fail(-1, "%s: 1 to %d triples per step, got %d", who, c.d_bsize, count);
  for (int t = 0; t < count; ++t)
    if (users[t] < 0 || users[t] >= h->U || pos_items[t] < 0 || pos_items[t] >= h->N || neg_items[t] < 0 || neg_items[t] >= h->N)
      return fail(-1, "%s: triple %d (%d, %d, %d) out of range", who, t, users[t], pos_items[t], neg_items[t]);
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  TRY(h->ca.loss_dev.grow(h->st, 1, true));
  HIP_TRY(hipStreamSynchronize(h->st));
  const int32_t* src[3] = {users, pos_items, neg_items};
  for (int q = 0; q < 3; ++q) HIP_TRY(hipMemcpy(c.xt + (size_t)q * c.d_bsize, src[q], (size_t)count * sizeof(int), hipMemcpyHostToDevice));
  TRY(caae_d_step(h, c.xt, c.xt + c.d_bsize, c.xt + 2 * (size_t)c.d_bsize, count, c.loss_dev));
  float l = 0.f;
  HIP_TRY(hipMemcpyAsync(&l, c.loss_dev, sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (loss) *loss = l;
  return 0;
}

int ganmf_caae_g_step(ganmf_handle* h, int which, const int32_t* users, const uint32_t* nu, const int32_t* items, float* loss) {
  const char* who = "ganmf_caae_g_step";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, true));
  if (which != 0 && which != 1) return fail(-1, "%s: which must be 0 (G) or 1 (G')", who);
  if (!users || !items) return fail(-1, "%s: null argument", who);
  CaaeState& c = h->ca;
  for (int b = 0; b < c.Bm; ++b)
    if (users[b] < 0 || users[b] >= h->U) return fail(-1, "%s: user %d out of range", who, users[b]);
  for (long long t = 0; t < (long long)c.Bm * c.n_s; ++t)
    if (items[t] < 0 || items[t] >= h->N) return fail(-1, "%s: item %d out of range", who, items[t]);
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  TRY(h->ca.loss_dev.grow(h->st, 1, true));
  HIP_TRY(hipStreamSynchronize(h->st));
  int* ud = c.xu;
  int* id = c.xi;
  unsigned* nd = c.xn;
  HIP_TRY(hipMemcpy(ud, users, (size_t)c.Bm * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(id, items, (size_t)c.Bm * c.n_s * sizeof(int), hipMemcpyHostToDevice));
  if (which == 0) {      // a null plane is cleared
    if (nu) HIP_TRY(hipMemcpy(nd, nu, (size_t)c.Bm * c.words * sizeof(unsigned), hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(nd, 0, (size_t)c.Bm * c.words * sizeof(unsigned)));
  }
  TRY(caae_g_step(h, which, ud, nd, id, c.loss_dev));
  float l = 0.f;
  HIP_TRY(hipMemcpyAsync(&l, c.loss_dev, sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (loss) *loss = l;
  return 0;
}

int ganmf_caae_epoch(ganmf_handle* h, int64_t epoch, int32_t d_steps, int32_t g_steps, int32_t gpr_steps, float* d_losses, float* g_losses,
                     float* gpr_losses) {
  const char* who = "ganmf_caae_epoch";
  TRY(model_ready(h, who, GANMF_MODEL_CAAE, true));
  if (d_steps < 0 || g_steps < 0 || gpr_steps < 0 || epoch < 0) return fail(-1, "%s: negative argument", who);
  CaaeState& c = h->ca;
  const long long nnz = h->urm.nnz;
  const size_t slices = (size_t)((nnz + c.d_bsize - 1) / c.d_bsize);
  const size_t nd = (size_t)d_steps * slices * 2, ng = (size_t)g_steps, np = (size_t)gpr_steps;
  if ((nd && !d_losses) || (ng && !g_losses) || (np && !gpr_losses)) return fail(-1, "%s: null loss buffer", who);
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  TRY(c.loss_dev.grow(h->st, nd + ng + np + 1, true));
  TRY(caae_prepare(h));
  TRY(caae_slots(h, d_steps, std::max(1, std::max(g_steps, gpr_steps))));
  c.rec_nnz = nnz; c.rec_passes = d_steps; c.rec_steps[0] = g_steps; c.rec_steps[1] = gpr_steps;
  // 1-2: the order, both generators over all users, both CDFs
  TRY(caae_draw_perm(h, epoch));
  TRY(caae_cdf_all(h, 0));
  TRY(caae_cdf_all(h, 1));
  float* out = c.loss_dev;
  // 3: discriminator passes: the pass's negatives from both CDFs, then per slice a step with G's and a step with G''s
  for (int pass = 0; pass < d_steps; ++pass) {
    int* ng_ = c.neg + (size_t)pass * 2 * std::max<long long>(nnz, 1);
    int* np_ = ng_ + std::max<long long>(nnz, 1);
    TRY(caae_draw_neg(h, epoch, pass, 0, ng_));
    TRY(caae_draw_neg(h, epoch, pass, 1, np_));
    for (long long s = 0; s < nnz; s += c.d_bsize) {
      const int cnt = (int)std::min<long long>(c.d_bsize, nnz - s);
      TRY(caae_d_step(h, c.tu + s, c.ti + s, ng_ + s, cnt, out++));
      TRY(caae_d_step(h, c.tu + s, c.ti + s, np_ + s, cnt, out++));
    }
  }
  // 4-5: generator steps, then the steps of G'
  for (int which = 0; which < 2; ++which)
    for (int step = 0; step < (which == 0 ? g_steps : gpr_steps); ++step) {
      int* ud = caae_users_slot(c, which, step);
      int* id = caae_items_slot(c, which, step);
      TRY(caae_draw_users(h, epoch, which, step, ud));
      if (which == 0) TRY(caae_draw_nu(h, epoch, step, ud, caae_nu_slot(c, step)));
      TRY(caae_draw_items(h, epoch, which, step, ud, id));
      TRY(caae_g_step(h, which, ud, caae_nu_slot(c, step), id, out++));
    }
  if (nd) HIP_TRY(hipMemcpyAsync(d_losses, c.loss_dev, nd * sizeof(float), hipMemcpyDeviceToHost, h->st));
  if (ng) HIP_TRY(hipMemcpyAsync(g_losses, c.loss_dev + nd, ng * sizeof(float), hipMemcpyDeviceToHost, h->st));
  if (np) HIP_TRY(hipMemcpyAsync(gpr_losses, c.loss_dev + nd + ng, np * sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}
