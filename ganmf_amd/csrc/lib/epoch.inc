// epoch.inc -- model dispatch, per-epoch loss arena, pinned staging, loss assembly
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// model dispatch
inline size_t arena_stride(const ganmf_handle* h) {      // floats per step: GANMF 4 segments of reg_cap, DisGANMF 5 + L of dis_cap
  return h->cfg.model == GANMF_MODEL_GANMF ? (size_t)4 * h->reg_cap : (size_t)(5 + h->L) * h->dis_cap;
}
int any_d_step(ganmf_handle* h, const int* rows_dev, int nb, int b_global, int64_t idx) {
  float* parts = h->d_parts + 4 * idx;
  float* slot = h->d_arena + (size_t)idx * arena_stride(h);
  if (h->cfg.model == GANMF_MODEL_GANMF) return d_step(h, rows_dev, nb, b_global, parts, slot);
  h->dis_slot = slot;
  return dis_d_step(h, rows_dev, nb, b_global, parts);
}
int any_g_step(ganmf_handle* h, const int* rows_dev, int nb, int start, int b_global, int64_t idx) {
  float* parts = h->g_parts + 4 * idx;
  float* slot = h->g_arena + (size_t)idx * arena_stride(h);
  if (h->cfg.model == GANMF_MODEL_GANMF) return g_step(h, rows_dev, nb, start, b_global, parts, slot);
  h->dis_slot = slot;
  return dis_g_step(h, rows_dev, nb, start, b_global, parts);
}

// zero the per-step arenas before a pass / reduce them into the loss parts after it (GANMF)
int ensure_parts(ganmf_handle* h, int64_t steps);
// Loss parts and per-step arenas of one call, packed into the front of parts_all and zeroed by ONE memset (the call starts on an
// idle queue: every separate fill costs its launch latency; a 20-step call is 2.6 ms of GPU work).
int parts_begin(ganmf_handle* h, int64_t nd, int64_t ng) {
  TRY(ensure_parts(h, std::max<int64_t>(std::max(nd, ng), 1)));
  const size_t stride = arena_stride(h);
  const size_t ndp = (size_t)std::max<int64_t>(nd, 1) * 4, ngp = (size_t)std::max<int64_t>(ng, 1) * 4;
  h->d_parts = h->parts_all;
  h->g_parts = h->d_parts + ndp;
  h->d_arena = h->g_parts + ngp;
  h->g_arena = h->d_arena + (size_t)std::max<int64_t>(nd, 0) * stride;
  const size_t total = ndp + ngp + (size_t)(std::max<int64_t>(nd, 0) + std::max<int64_t>(ng, 0)) * stride;
  HIP_TRY(hipMemsetAsync(h->parts_all, 0, total * sizeof(float), h->st));
  return 0;
}
int arenas_finish(ganmf_handle* h, int64_t nd, int64_t ng) {
  const size_t stride = arena_stride(h);
  Scope s(h, T_MULTIRED, 0, 4.0 * (nd + ng) * stride);
  if (h->cfg.model == GANMF_MODEL_GANMF) {
    if (nd > 0) GANMF_LAUNCH(finish_parts_kernel, dim3((int)nd), dim3(256), 0, h->st, h->d_arena, h->reg_cap, 0, h->d_parts);
    if (ng > 0) GANMF_LAUNCH(finish_parts_kernel, dim3((int)ng), dim3(256), 0, h->st, h->g_arena, h->reg_cap, 1, h->g_parts);
  } else {
    if (nd > 0) GANMF_LAUNCH(finish_dis_parts_kernel, dim3((int)nd), dim3(256), 0, h->st, h->d_arena, (long long)stride, h->dis_cap, 5 + h->L, 0, h->d_parts);
    if (ng > 0) GANMF_LAUNCH(finish_dis_parts_kernel, dim3((int)ng), dim3(256), 0, h->st, h->g_arena, (long long)stride, h->dis_cap, 5 + h->L, 1, h->g_parts);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// pinned host staging (ints: permutation | inverse permutation; floats: loss parts), grown on demand
int ensure_stage(ganmf_handle* h, size_t n_int, size_t n_float) {
  if (n_int > h->stage_i.cap) TRY(h->stage_i.alloc(n_int, false));
  if (n_float > h->stage_f.cap) TRY(h->stage_f.alloc(n_float + n_float / 2 + 256, false));
  return 0;
}

int ensure_parts(ganmf_handle* h, int64_t steps) {
  if (steps <= (int64_t)h->colbuf.cap) return 0;      // (colbuf, allocated last, holds one float per step of room)
  HIP_TRY(hipStreamSynchronize(h->st));
  // a failing allocation leaves colbuf empty and null views, so the next call allocates again instead of running on freed memory
  h->parts_all.reset(); h->colbuf.reset();
  h->d_parts = h->g_parts = h->d_arena = h->g_arena = nullptr;
  const int64_t cap = steps + 64;
  TRY(h->parts_all.alloc((size_t)cap * 2 * (4 + arena_stride(h)), true));
  TRY(h->colbuf.alloc((size_t)cap, true));
  return 0;
}

// losses from the per-step parts (fp32 host arithmetic, same expression order as the oracle)
void finish_losses(const ganmf_handle* h, const std::vector<float>& dp, const std::vector<float>& gp,
                   const std::vector<int>& bglob, int64_t nd, int64_t ng, int64_t per_pass, float* d_losses,
                   float* g_losses) {
  const float alpha = h->cfg.recon_coefficient;
  if (h->cfg.model == GANMF_MODEL_DISGANMF) {
    for (int64_t i = 0; i < nd && d_losses; ++i) {
      const float bg = (float)bglob[i % per_pass];
      const float sq = dp[4 * i + 2];     // (data-parallel: every rank summed its own slice; all-reduced = the whole tensor)
      d_losses[i] = (dp[4 * i] / bg + dp[4 * i + 1] / bg) + h->cfg.d_reg * (sq / 2.0f);
    }
    for (int64_t i = 0; i < ng && g_losses; ++i) {
      const float bg = (float)bglob[i % per_pass];
      const float sv = gp[4 * i + 3];
      g_losses[i] = (gp[4 * i] / bg + alpha * (gp[4 * i + 1] / (bg * (float)h->e))) + h->cfg.g_reg * ((gp[4 * i + 2] + sv) / 2.0f);
    }
    return;
  }
  for (int64_t i = 0; i < nd && d_losses; ++i)
    d_losses[i] = dp[4 * i] + h->cfg.d_reg * (dp[4 * i + 2] / 2.0f);
  for (int64_t i = 0; i < ng && g_losses; ++i) {
    const float bg = (float)bglob[i % per_pass];
    const float Lf = gp[4 * i] / (bg * (float)h->N);
    const float fm = gp[4 * i + 1] / (bg * (float)h->e);
    const float sv = gp[4 * i + 3];       // (data-parallel: slices of V, all-reduced)
    g_losses[i] = ((1.0f - alpha) * Lf + alpha * fm) + h->cfg.g_reg * ((gp[4 * i + 2] + sv) / 2.0f);
  }
}

