// abi_train.inc -- C ABI: ganmf_train_epoch / _ragged / ganmf_train_step
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
int ganmf_train_epoch(ganmf_handle* h, const int32_t* perm, int64_t n, int32_t d_steps, int32_t g_steps,
                      int64_t n_steps_per_pass, const int32_t* global_batch_rows, float* d_losses,
                      float* g_losses) {
  return ganmf_train_epoch_ragged(h, perm, n, d_steps, g_steps, n_steps_per_pass, global_batch_rows, nullptr, d_losses, g_losses);
}

int ganmf_train_epoch_ragged(ganmf_handle* h, const int32_t* perm, int64_t n, int32_t d_steps, int32_t g_steps,
                             int64_t n_steps_per_pass, const int32_t* global_batch_rows,
                             const int32_t* local_batch_rows, float* d_losses, float* g_losses) {
  if (!h || (!perm && n > 0)) return fail(-1, "ganmf_train_epoch: null argument");
  TRY(needs_tensors(h, "ganmf_train_epoch"));
  TRY(not_cfgan(h, "ganmf_train_epoch"));
  if (h->cfg.model == GANMF_MODEL_MF) return fail(-1, "ganmf_train_epoch: a GANMF_MODEL_MF handle holds factors only and has no adversarial training; its factors come from ganmf_als_half_sweep or ganmf_set_tensor");
  if (!h->has_urm) return fail(-1, "ganmf_train_epoch: ganmf_set_urm_csr has not been called");
  if (n < 0 || n > h->U) return fail(-1, "ganmf_train_epoch: n=%lld out of range", (long long)n);
  if (d_steps < 0 || g_steps < 0) return fail(-1, "ganmf_train_epoch: negative step count");
  const bool dist = h->has_comm && h->cfg.world_size > 1;
  if (dist && !global_batch_rows) return fail(-1, "ganmf_train_epoch: global_batch_rows required when world_size > 1");
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  prealloc_pass_buffers(h, local_batch_rows != nullptr);
  const int B = h->B;
  const int64_t local_steps = local_batch_rows ? n_steps_per_pass : (n + B - 1) / B;
  const int64_t per_pass = std::max(local_steps, n_steps_per_pass);
  if (per_pass == 0) return 0;
  // slice i = rows [slice_at[i], slice_at[i] + slice_nb[i]) of the permutation
  std::vector<int64_t> slice_at(per_pass);
  std::vector<int> slice_nb(per_pass);
  {
    int64_t at = 0;
    for (int64_t i = 0; i < per_pass; ++i) {
      int nb;
      if (local_batch_rows) {
        nb = local_batch_rows[i];
        if (nb < 0 || nb > B || at + nb > n) return fail(-1, "ganmf_train_epoch_ragged: local_batch_rows[%lld]=%d (batch_size %d, %lld of %lld rows used)", (long long)i, nb, B, (long long)at, (long long)n);
      } else {
        nb = (int)std::max<int64_t>(0, std::min<int64_t>(B, n - i * B));
        at = std::min<int64_t>(i * B, n);
      }
      slice_at[i] = at; slice_nb[i] = nb;
      at += nb;
    }
    if (local_batch_rows && at != n) return fail(-1, "ganmf_train_epoch_ragged: local_batch_rows sum to %lld, n = %lld", (long long)at, (long long)n);
  }
  // the permutation and its inverse go up from ONE pinned staging buffer in one asynchronous copy, the loss parts come back
  // into pinned memory: pageable copies are staged synchronously by the runtime, ~0.1 ms per epoch call that a 10-slice call
  // (2.6 ms of GPU work) notices
  TRY(ensure_stage(h, (size_t)3 * h->U, 0));
  int* const stage_perm = h->stage_i;
  int* const pos = h->stage_i + h->U;
  int* const pos_step = h->stage_i + 2 * (size_t)h->U;      // step (slice) index of every schedule position
  std::fill(pos, pos + h->U, -1);
  for (int64_t i = 0; i < per_pass; ++i) std::fill(pos_step + slice_at[i], pos_step + slice_at[i] + slice_nb[i], (int)i);
  for (int64_t i = 0; i < n; ++i) {
    const int r = perm[i];
    if (r < 0 || r >= h->U) return fail(-1, "ganmf_train_epoch: row id %d out of range at %lld", r, (long long)i);
    if (pos[r] != -1) return fail(-1, "ganmf_train_epoch: row id %d appears twice in the permutation", r);
    pos[r] = (int)i;
    stage_perm[i] = r;
  }
  std::vector<int> bglob(per_pass);
  for (int64_t i = 0; i < per_pass; ++i) {
    const int nb = slice_nb[i];
    bglob[i] = global_batch_rows ? global_batch_rows[i] : nb;
    if (bglob[i] < nb || bglob[i] < 1) return fail(-1, "ganmf_train_epoch: global_batch_rows[%lld]=%d < local %d", (long long)i, bglob[i], nb);
  }
  HIP_TRY(hipMemcpyAsync(h->perm, stage_perm, (size_t)3 * h->U * sizeof(int), hipMemcpyHostToDevice, h->st));   // perm | pos | pos_step, contiguous on both sides
  const int64_t nd = (int64_t)d_steps * per_pass, ng = (int64_t)g_steps * per_pass;
  TRY(parts_begin(h, nd, ng));
  // Discriminator passes.  U, V and the URM do not change while they run: the row expansion and the generated rows of every full
  // minibatch are formed once, in front of them (stage_pass); minibatch i then reads its [real ; generated] block and its own lr_t slot.
  const int64_t nfull = (local_batch_rows || d_steps == 0) ? 0 : n / B;
  GemmPlan stage_pl{};
  bool stage_front = false;
  const bool staged = nfull > 0 && stage_pass_plan(h, nfull, &stage_pl, &stage_front);
  const bool lazy = g_steps > 0 && lazy_pass_ok(h, per_pass, n);      // (generator passes, below)
  // The generator passes walk the same slices of the same shuffle (GANMF.py:175-203): their real rows are the X halves of the staged blocks.
  // A call without discriminator passes stages the rows alone.  (Dense generator path with the per-pass update of U only; GANMF_TUNE g_rows_staged=0:
  // every generator step expands its own rows.)
  // Only where a generator step's row expansion is a launch of its own (wide rows: the configs[3] shard, 19.8 us of a 200 us step): where it
  // rides in the generator GEMM's launch (front_kernel: ML-1M, configs[4]) it costs nothing and leaves the rows in L2 for the encode GEMM --
  // staged rows measured 2 % slower there.  g_rows_staged = 2: staged wherever possible (tests).
  bool gen_front = false;
  if (g_steps > 0 && h->g_rows_staged == 1) (void)generator_plan(h, B, &gen_front);
  const int64_t nfull_g = (local_batch_rows || g_steps == 0 || !lazy || h->sparse_g || !h->g_rows_staged || gen_front) ? 0 : n / B;
  GemmPlan gonly_pl{};
  bool gonly_front = false;
  const bool rows_only = !staged && d_steps == 0 && nfull_g > 0 && !h->sparse_d && stage_pass_plan(h, nfull_g, &gonly_pl, &gonly_front);
  const bool gx = nfull_g > 0 && (staged || rows_only);
  // Whatever way this call ends, the handle is left with its own minibatch buffers, lr_t slots and no open per-pass state; and when the
  // staged row expansion has opened the first generator pass's steps ahead of time (the beta powers advance with them) but a
  // discriminator step fails before that pass starts, the generator's powers go back to what they were.
  struct PassGuard {
    ganmf_handle* h;
    bool g_opened_early = false;
    ~PassGuard() {
      h->front_staged = false; h->x_staged = false; h->XF = h->XF_own; h->d_alpha = S_ALPHA_D;
      if (h->lazy_pass) lazy_pass_abort(h);
      if (g_opened_early) {
        GANMF_LAUNCH(restore_g_powers_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get());
        (void)hipGetLastError();
      }
    }
  } guard{h};
  if (staged) {
    const bool dis = h->cfg.model == GANMF_MODEL_DISGANMF;
    TRY(stage_pass(h, h->perm, nfull, stage_pl, stage_front, dis ? h->N + 1 : -1, dis ? (int)h->cfg.row_offset : 0, lazy ? (int)per_pass : 0,
                   &guard.g_opened_early));
  } else if (rows_only) {
    const bool dis = h->cfg.model == GANMF_MODEL_DISGANMF;
    TRY(stage_pass(h, h->perm, nfull_g, gonly_pl, gonly_front, dis ? h->N + 1 : -1, dis ? (int)h->cfg.row_offset : 0, 0, nullptr, /*gen=*/false));
  }
  int64_t idx = 0;
  for (int p = 0; p < d_steps; ++p) {
    const int tab = S_TAB + (p & 1) * h->tab_cap;      // (passes alternate tables: a side-lane update of the pass before may still read its slot)
    if (staged && p > 0) {      // (the first pass's table was written by stage_pass's row-expansion launch)
      GANMF_LAUNCH(open_steps_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get(), 0, tab, (int)nfull, h->cfg.d_lr);
      HIP_TRY(hipGetLastError());
    }
    for (int64_t i = 0; i < per_pass; ++i, ++idx) {
      const int64_t a = slice_at[i];
      const int nb = slice_nb[i];
      const bool st = staged && i < nfull;
      h->front_staged = st;
      h->XF = st ? h->XF_pass + (size_t)i * 2 * B * h->ldN : h->XF_own;
      if (st) h->d_alpha = tab + (int)i;
      else if (staged) h->d_alpha = S_ALPHA_D;
      TRY(any_d_step(h, h->perm + std::min<int64_t>(a, std::max<int64_t>(n - 1, 0)), nb, bglob[i], idx));
    }
  }
  if (staged) { h->front_staged = false; h->XF = h->XF_own; h->d_alpha = S_ALPHA_D; }
  // Generator passes.  With g_reg == 0 a row of U is read once and receives a gradient once per pass: the all-rows Adam over U runs
  // once per pass (lazy_pass_begin / lazy_pass_end, step_ganmf.inc) instead of once per step.
  idx = 0;
  for (int p = 0; p < g_steps; ++p) {
    if (lazy) TRY(lazy_pass_begin(h, p, per_pass, n, staged && p == 0));
    guard.g_opened_early = false;      // (the steps those powers belong to are running now)
    for (int64_t i = 0; i < per_pass; ++i, ++idx) {
      const int64_t a = slice_at[i];
      const int nb = slice_nb[i];
      if (lazy) { h->lazy_step = (int)i; h->g_alpha = lazy_tab_slot(h, p) + (int)i; h->Ub = h->Ub_sched + (size_t)std::min<int64_t>(a, std::max<int64_t>(n - 1, 0)) * h->ldk; }
      const bool xst = gx && i < nfull_g;
      h->x_staged = xst;
      h->XF = xst ? h->XF_pass + (size_t)i * 2 * B * h->ldN : h->XF_own;
      TRY(any_g_step(h, h->perm + std::min<int64_t>(a, std::max<int64_t>(n - 1, 0)), nb, (int)a, bglob[i], idx));
    }
    if (lazy) TRY(lazy_pass_end(h, p, per_pass));
  }
  h->x_staged = false; h->XF = h->XF_own;
  TRY(dp_join(h));      // the last step's side-lane updates (and their sum(theta^2) partials) are complete
  TRY(arenas_finish(h, nd, ng));
  // loss parts are sums over this rank's rows / this rank's slices of the replicated tensors: one all-reduce per epoch.
  // GANMF's D loss itself (column 0) is formed on the device from sums that were all-reduced before the hinge and is
  // global already: only its sum(theta_D^2) column travels.
  if (dist && nd > 0) {
    if (h->cfg.model == GANMF_MODEL_DISGANMF) TRY(allreduce(h, h->d_parts, (size_t)nd * 4));
    else {
      const int grid = (int)std::min<int64_t>(256, (nd + 255) / 256);
      GANMF_LAUNCH(col_copy_kernel, dim3(grid), dim3(256), 0, h->st, h->d_parts, h->colbuf.get(), (long long)nd, 2, 1);
      HIP_TRY(hipGetLastError());
      TRY(allreduce(h, h->colbuf, (size_t)nd));
      GANMF_LAUNCH(col_copy_kernel, dim3(grid), dim3(256), 0, h->st, h->d_parts, h->colbuf.get(), (long long)nd, 2, 0);
      HIP_TRY(hipGetLastError());
    }
  }
  if (dist && ng > 0) TRY(allreduce(h, h->g_parts, (size_t)ng * 4));
  const size_t ndp = (size_t)std::max<int64_t>(nd, 1) * 4, ngp = (size_t)std::max<int64_t>(ng, 1) * 4;
  TRY(ensure_stage(h, 0, ndp + ngp));
  HIP_TRY(hipMemcpyAsync(h->stage_f, h->d_parts, (ndp + ngp) * sizeof(float), hipMemcpyDeviceToHost, h->st));   // d_parts | g_parts, contiguous
  HIP_TRY(hipStreamSynchronize(h->st));
  const float* const sf = h->stage_f;
  const std::vector<float> dp(sf, sf + ndp), gp(sf + ndp, sf + ndp + ngp);
  finish_losses(h, dp, gp, bglob, nd, ng, per_pass, d_losses, g_losses);
  return 0;
}

int ganmf_train_step(ganmf_handle* h, int kind, const int32_t* uids, int32_t n, float* loss) {
  if (!h || !uids) return fail(-1, "ganmf_train_step: null argument");
  TRY(needs_tensors(h, "ganmf_train_step"));
  TRY(not_cfgan(h, "ganmf_train_step"));
  if (h->cfg.model == GANMF_MODEL_MF) return fail(-1, "ganmf_train_step: a GANMF_MODEL_MF handle holds factors only and has no adversarial training; its factors come from ganmf_als_half_sweep or ganmf_set_tensor");
  if (!h->has_urm) return fail(-1, "ganmf_train_step: ganmf_set_urm_csr has not been called");
  if (n < 1 || n > h->B) return fail(-1, "ganmf_train_step: batch of %d rows (handle batch_size %d)", n, h->B);
  if (kind != 0 && kind != 1) return fail(-1, "ganmf_train_step: kind must be 0 (D) or 1 (G)");
  if (h->has_comm && h->cfg.world_size > 1) return fail(-1, "ganmf_train_step: single-GPU entry; use ganmf_train_epoch");
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  std::vector<int> pos(h->U, -1);
  for (int i = 0; i < n; ++i) {
    if (uids[i] < 0 || uids[i] >= h->U) return fail(-1, "ganmf_train_step: row id %d out of range", uids[i]);
    if (pos[uids[i]] != -1) return fail(-1, "ganmf_train_step: duplicate row id %d", uids[i]);
    pos[uids[i]] = i;
  }
  HIP_TRY(hipMemcpyAsync(h->perm, uids, n * sizeof(int), hipMemcpyHostToDevice, h->st));
  HIP_TRY(hipMemcpyAsync(h->pos, pos.data(), (size_t)h->U * sizeof(int), hipMemcpyHostToDevice, h->st));
  TRY(parts_begin(h, kind == 0, kind == 1));
  if (kind == 0) TRY(any_d_step(h, h->perm, n, n, 0));
  else TRY(any_g_step(h, h->perm, n, 0, n, 0));
  TRY(dp_join(h));
  TRY(arenas_finish(h, kind == 0, kind == 1));
  std::vector<float> dp(4), gp(4);
  HIP_TRY(hipMemcpyAsync(dp.data(), h->d_parts, 4 * sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipMemcpyAsync(gp.data(), h->g_parts, 4 * sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  std::vector<int> bglob(1, n);
  float dl = 0.f, gl = 0.f;
  finish_losses(h, dp, gp, bglob, kind == 0 ? 1 : 0, kind == 1 ? 1 : 0, 1, &dl, &gl);
  if (loss) *loss = kind == 0 ? dl : gl;
  return 0;
}

