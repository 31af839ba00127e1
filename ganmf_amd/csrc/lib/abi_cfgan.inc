// abi_cfgan.inc -- C ABI: CFGAN on a GANMF_MODEL_CFGAN handle: ganmf_cfgan_init / _draw_masks / _set_masks / _get_masks / _step / _epoch
// (cfgan_masks.hpp, cfgan_rows.hpp, step_cfgan.inc)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

int ganmf_cfgan_init(ganmf_handle* h, int32_t g_nodes, int32_t g_layers, int g_act, int32_t d_batch, int32_t g_batch, int scheme,
                     float zr_coefficient, uint64_t seed, const int32_t* k_rows) {
  const char* who = "ganmf_cfgan_init";
  if (!h || !k_rows) return fail(-1, "%s: null argument", who);
  if (h->cfg.model != GANMF_MODEL_CFGAN) return fail(-1, "%s: needs a GANMF_MODEL_CFGAN handle", who);
  if (h->cf.ready) return fail(-1, "%s: the handle is initialised already", who);
  if (g_nodes < 1 || g_layers < 1 || g_layers > 16 || g_act < 0 || g_act > 3)
    return fail(-1, "%s: needs g_nodes >= 1, 1 <= g_layers <= 16 and a known activation", who);
  if (scheme != GANMF_CFGAN_ZR && scheme != GANMF_CFGAN_PM && scheme != GANMF_CFGAN_ZP) return fail(-1, "%s: unknown scheme %d", who, scheme);
  if (d_batch < 1 || g_batch < 1) return fail(-1, "%s: non-positive batch size", who);
  if (!std::isfinite(zr_coefficient)) return fail(-1, "%s: zr_coefficient must be finite", who);
  const int U = h->U, N = h->N;
  const int Bm = std::max(std::min(d_batch, U), std::min(g_batch, U));
  if (Bm > h->B) return fail(-1, "%s: the handle was created for batches of %d rows, asked for %d", who, h->B, Bm);
  for (int u = 0; u < U; ++u)
    if (k_rows[u] < 0 || k_rows[u] > N) return fail(-1, "%s: k_rows[%d] = %d out of range [0,%d]", who, u, k_rows[u], N);
  HIP_TRY(hipSetDevice(h->dev));
  CfganState& c = h->cf;
  c.d_batch = std::min(d_batch, U); c.g_batch = std::min(g_batch, U); c.Bm = Bm; c.scheme = scheme;
  c.zr_coef = zr_coefficient; c.seed = seed;
  c.ldx = round_up(2 * N + 2, LD_ALIGN); c.words = (N + 31) / 32;
  TRY(mlp_alloc(h, c.gen, g_nodes, g_layers, g_act, -1, Bm));
  TRY(c.C.alloc((size_t)Bm * h->ldN, true));
  TRY(c.fake.alloc((size_t)Bm * h->ldN, true));
  TRY(c.dfake.alloc((size_t)Bm * h->ldN, true));
  TRY(c.DX.alloc((size_t)2 * Bm * c.ldx, true));
  TRY(c.dh0.alloc((size_t)Bm * c.gen.ldg, true));
  TRY(c.dh1.alloc((size_t)Bm * c.gen.ldg, true));
  TRY(c.zr_part.alloc((size_t)Bm, true));
  TRY(c.loss_rows.alloc((size_t)2 * Bm, true));
  TRY(c.sq.alloc((size_t)(std::max(h->L, g_layers) + 1) * CFGAN_SQ_BLOCKS, true));
  TRY(c.planes.alloc((size_t)2 * U * c.words, true));
  TRY(c.k_rows.alloc((size_t)U, true));
  HIP_TRY(hipMemcpy(c.k_rows, k_rows, (size_t)U * sizeof(int), hipMemcpyHostToDevice));
  c.ready = true;
  ++h->param_version;
  return 0;
}

static int cfgan_draw(ganmf_handle* h, int64_t epoch) {
  CfganState& c = h->cf;
  CfganMaskP p{h->urm.indptr, h->urm.indices, c.k_rows, h->U, h->N, c.words, c.seed, (unsigned long long)epoch, c.planes,
               c.scheme == GANMF_CFGAN_PM ? CFGAN_PLANE_PM : CFGAN_PLANE_ZR};
  GANMF_LAUNCH(cfgan_masks_kernel, dim3(h->U, c.scheme == GANMF_CFGAN_ZP ? 2 : 1), dim3(256), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

int ganmf_cfgan_draw_masks(ganmf_handle* h, int64_t epoch) {
  const char* who = "ganmf_cfgan_draw_masks";
  TRY(model_ready(h, who, GANMF_MODEL_CFGAN, true));
  if (epoch < 0) return fail(-1, "%s: negative epoch", who);
  HIP_TRY(hipSetDevice(h->dev));
  TRY(cfgan_draw(h, epoch));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}

int ganmf_cfgan_set_masks(ganmf_handle* h, const uint32_t* zr, const uint32_t* pm) {
  TRY(model_ready(h, "ganmf_cfgan_set_masks", GANMF_MODEL_CFGAN, false));
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  const size_t n = (size_t)h->U * h->cf.words;
  const uint32_t* src[2] = {zr, pm};
  for (int q = 0; q < 2; ++q) {      // a null plane is cleared
    if (src[q]) HIP_TRY(hipMemcpy(h->cf.planes + q * n, src[q], n * sizeof(uint32_t), hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(h->cf.planes + q * n, 0, n * sizeof(uint32_t)));
  }
  return 0;
}

int ganmf_cfgan_get_masks(ganmf_handle* h, uint32_t* zr, uint32_t* pm) {
  TRY(model_ready(h, "ganmf_cfgan_get_masks", GANMF_MODEL_CFGAN, false));
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  const size_t n = (size_t)h->U * h->cf.words;
  if (zr) HIP_TRY(hipMemcpy(zr, h->cf.planes, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (pm) HIP_TRY(hipMemcpy(pm, h->cf.planes + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_cfgan_step(ganmf_handle* h, int kind, int64_t row0, int32_t nrows, float* loss) {
  const char* who = "ganmf_cfgan_step";
  TRY(model_ready(h, who, GANMF_MODEL_CFGAN, true));
  if (kind != 0 && kind != 1) return fail(-1, "%s: kind must be 0 (D) or 1 (G)", who);
  if (nrows < 1 || nrows > h->cf.Bm || row0 < 0 || row0 + nrows > h->U)
    return fail(-1, "%s: rows [%lld, %lld) of %d, at most %d per step", who, (long long)row0, (long long)row0 + nrows, h->U, h->cf.Bm);
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  TRY(h->cf.loss_dev.grow(h->st, 1, true));
  TRY(cfgan_step(h, kind, (int)row0, nrows, h->cf.loss_dev));
  float l = 0.f;
  HIP_TRY(hipMemcpyAsync(&l, h->cf.loss_dev, sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (loss) *loss = l;
  return 0;
}

int ganmf_cfgan_epoch(ganmf_handle* h, int64_t epoch, int32_t d_steps, int32_t g_steps, int draw, float* d_losses, float* g_losses) {
  const char* who = "ganmf_cfgan_epoch";
  TRY(model_ready(h, who, GANMF_MODEL_CFGAN, true));
  if (d_steps < 0 || g_steps < 0 || epoch < 0) return fail(-1, "%s: negative argument", who);
  CfganState& c = h->cf;
  const int U = h->U;
  const size_t nd = (size_t)d_steps * ((U + c.d_batch - 1) / c.d_batch), ng = (size_t)g_steps * ((U + c.g_batch - 1) / c.g_batch);
  if ((nd && !d_losses) || (ng && !g_losses)) return fail(-1, "%s: null loss buffer", who);
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  TRY(c.loss_dev.grow(h->st, nd + ng + 1, true));
  if (draw) TRY(cfgan_draw(h, epoch));
  float* out = c.loss_dev;
  for (int pass = 0; pass < d_steps; ++pass)
    for (int r0 = 0; r0 < U; r0 += c.d_batch) TRY(cfgan_step(h, 0, r0, std::min(c.d_batch, U - r0), out++));
  for (int pass = 0; pass < g_steps; ++pass)
    for (int r0 = 0; r0 < U; r0 += c.g_batch) TRY(cfgan_step(h, 1, r0, std::min(c.g_batch, U - r0), out++));
  if (nd) HIP_TRY(hipMemcpyAsync(d_losses, c.loss_dev, nd * sizeof(float), hipMemcpyDeviceToHost, h->st));
  if (ng) HIP_TRY(hipMemcpyAsync(g_losses, c.loss_dev + nd, ng * sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}
