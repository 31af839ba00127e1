// step_caae.inc -- CAAE: the two generators' CDFs, the draws, the D-step, the G / G' step, scoring (CAAE.py:47-119,215-337,382-395)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// =================================================================================================
// Discriminator: P = h->Ue, Q = h->V, b = CaaeState::bias; plain SGD on the touched rows (caae_rows.hpp).  Generators: CaaeState::gen[0]
// (G) and gen[1] (G'), sigmoid on every layer.  Every dense product goes through run_gemm under the handle's planner: the forward and
// backward passes are the shared generator's (profile_mlp.inc, the sigmoid on the output layer too), and every parameter gradient runs
// as a TN product that stores into the tensor's own gradient buffer (EPI_STORE); caae_sgd_kernel then applies
// theta -= lr * (g + beta * theta).  Products that read a parameter run before the kernel that updates it.  sum(theta^2) of the loss is
// taken at the head of the step, at the pre-update parameters like every other term of the reported loss.
// =================================================================================================
// The fourth score source behind scores_device: out[i, :] = sigmoid(G(profile of ids[i])) -- the sigmoid applied, as CAAE.py:391 returns it
int caae_scores(ganmf_handle* h, const int* ids_dev, int64_t n, int transposed, float* out, int ldw) {
  if (!h->ca.ready) return fail(-1, "scores: ganmf_caae_init has not been called on this GANMF_MODEL_CAAE handle");
  if (!h->has_urm) return fail(-1, "scores: ganmf_set_urm_csr has not been called");
  if (transposed) return fail(-1, "scores: a GANMF_MODEL_CAAE handle scores users only (the reference ignores `mode`)");
  return mlp_forward_rows(h, h->ca.gen[0], ids_dev, 0, (int)n, out, ldw);
}

constexpr int CAAE_ALL_BLOCK = 1024;

// resident CDF of generator `which` over all users, block by block (CAAE.py:228-241)
int caae_cdf_all(ganmf_handle* h, int which) {
  CaaeState& c = h->ca;
  ProfileMlp& gn = c.gen[which];
  const int U = h->U, blk = std::min(U, CAAE_ALL_BLOCK);
  TRY(mlp_scratch(h, gn, (size_t)blk));      // grown here: sc_F is named as the output below, before mlp_forward_rows would grow it
  for (int r0 = 0; r0 < U; r0 += blk) {
    const int nb = std::min(blk, U - r0);
    TRY(mlp_forward_rows(h, gn, nullptr, r0, nb, gn.sc_F, h->ldN));
    GANMF_LAUNCH(caae_cdf_rows_kernel, dim3(nb), dim3(256), 0, h->st, gn.sc_F.get(), h->ldN, h->N, c.cdf[which] + (size_t)r0 * h->ldN, h->ldN,
                 c.lse_all + r0);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// iu (the user of every CSR position) and the shuffled-order buffers for the URM held now
int caae_prepare(ganmf_handle* h) {
  CaaeState& c = h->ca;
  if (c.iu_src == (const void*)h->urm.indptr && (long long)c.ti.cap >= h->urm.nnz) return 0;      // (ti is allocated last)
  HIP_TRY(hipStreamSynchronize(h->st));
  c.iu.reset(); c.perm.reset(); c.tu.reset(); c.ti.reset();
  c.iu_src = nullptr;
  const size_t n = (size_t)std::max<long long>(h->urm.nnz, 1);
  TRY(c.iu.alloc(n, true));
  TRY(c.perm.alloc(n, true));
  TRY(c.tu.alloc(n, true));
  TRY(c.ti.alloc(n, true));
  GANMF_LAUNCH(caae_rows_of_kernel, dim3(h->U), dim3(256), 0, h->st, h->urm.indptr.get(), h->U, c.iu.get());
  HIP_TRY(hipGetLastError());
  c.iu_src = (const void*)h->urm.indptr;
  return 0;
}

inline int caae_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>(4096, (n + 255) / 256)); }

// (a) the epoch's order and its (user, item) pairs
int caae_draw_perm(ganmf_handle* h, int64_t epoch) {
  CaaeState& c = h->ca;
  TRY(caae_prepare(h));
  if (h->urm.nnz == 0) return 0;
  GANMF_LAUNCH(caae_perm_kernel, dim3(caae_grid(h->urm.nnz)), dim3(256), 0, h->st, caae_base(c.seed, (unsigned long long)epoch, CAAE_S_PERM, 0),
               h->urm.nnz, c.iu.get(), h->urm.indices.get(), c.perm.get(), c.tu.get(), c.ti.get());
  HIP_TRY(hipGetLastError());
  return 0;
}

// (b) one negative per position from the resident CDF of generator `which`
int caae_draw_neg(ganmf_handle* h, int64_t epoch, int pass, int which, int* out) {
  CaaeState& c = h->ca;
  if (h->urm.nnz == 0) return 0;
  GANMF_LAUNCH(caae_cdf_draw_kernel, dim3(caae_grid(h->urm.nnz)), dim3(256), 0, h->st,
               caae_base(c.seed, (unsigned long long)epoch, CAAE_S_NEG + which, (unsigned long long)pass), h->urm.nnz, c.tu.get(), 1, c.cdf[which].get(), h->ldN, h->N, out);
  HIP_TRY(hipGetLastError());
  return 0;
}

// (c)
int caae_draw_users(ganmf_handle* h, int64_t epoch, int which, int step, int* out) {
  CaaeState& c = h->ca;
  GANMF_LAUNCH(caae_users_kernel, dim3((c.Bm + 255) / 256), dim3(256), 0, h->st,
               caae_base(c.seed, (unsigned long long)epoch, CAAE_S_USERS + which, (unsigned long long)step), c.Bm, h->U, which == 0 ? 1 : 0, out);
  HIP_TRY(hipGetLastError());
  return 0;
}

// forward of generator `which` over the batch's rows into R (or Rp), hidden outputs into the generator's own blocks
int caae_batch_forward(ganmf_handle* h, int which, const int* users_dev, float* out) {
  return mlp_forward_rows(h, h->ca.gen[which], users_dev, 0, h->ca.Bm, out, h->ldN, h->ca.C);
}

// (d) the Nu planes of the batch's rows, weighted by G' at its current parameters (inside an epoch: its epoch-start parameters, because
// G' only moves in the steps behind the generator steps)
int caae_draw_nu(ganmf_handle* h, int64_t epoch, int step, const int* users_dev, unsigned* planes) {
  CaaeState& c = h->ca;
  TRY(caae_batch_forward(h, 1, users_dev, c.Rp));
  CaaeNuP p{h->urm.indptr, h->urm.indices, users_dev, c.k_rows, c.Rp, h->ldN, h->N, c.words,
            caae_base(c.seed, (unsigned long long)epoch, CAAE_S_NU, (unsigned long long)step), planes};
  GANMF_LAUNCH(caae_nu_kernel, dim3(c.Bm), dim3(256), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// (e) n_s items per batch row from the CDF of generator `which` over the batch's rows (left in cdfb)
int caae_draw_items(ganmf_handle* h, int64_t epoch, int which, int step, const int* users_dev, int* items) {
  CaaeState& c = h->ca;
  TRY(caae_batch_forward(h, which, users_dev, c.R));
  GANMF_LAUNCH(caae_cdf_rows_kernel, dim3(c.Bm), dim3(256), 0, h->st, c.R.get(), h->ldN, h->N, c.cdfb.get(), h->ldN, c.lse.get());
  HIP_TRY(hipGetLastError());
  const long long n = (long long)c.Bm * c.n_s;
  GANMF_LAUNCH(caae_cdf_draw_kernel, dim3(caae_grid(n)), dim3(256), 0, h->st,
               caae_base(c.seed, (unsigned long long)epoch, CAAE_S_ITEMS + which, (unsigned long long)step), n, (const int*)nullptr, c.n_s, c.cdfb.get(),
               h->ldN, h->N, items);
  HIP_TRY(hipGetLastError());
  return 0;
}

// One discriminator step on cnt triples (device arrays); the slice's loss -> *loss_dev
int caae_d_step(ganmf_handle* h, const int* tu, const int* ti, const int* tj, int cnt, float* loss_dev) {
  CaaeState& c = h->ca;
  CaaeDP p{tu, ti, tj, cnt, h->k, h->ldk, h->Ue.p, h->V.p, c.bias.p, c.Pg, c.Qi, c.Qj, c.coef, c.lt, c.rt, c.rt + c.d_bsize, c.first, h->U, c.lr, c.beta};
  GANMF_LAUNCH(caae_d_coef_kernel, dim3((cnt + 3) / 4), dim3(256), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  GANMF_LAUNCH(cfgan_loss_kernel, dim3(1), dim3(256), 0, h->st, c.lt.get(), (const float*)nullptr, cnt, c.rt.get(), cnt, c.beta, (const float*)nullptr, 0.f, loss_dev);
  HIP_TRY(hipGetLastError());
  GANMF_LAUNCH(caae_d_update_kernel, dim3((3 * cnt + 3) / 4), dim3(256), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// dW = A_ext^T . dz over `nrows` rows into the tensor's own gradient buffer
int caae_wgrad(ganmf_handle* h, const float* A, int lda, const float* dz, int ldz, Tensor& W, int M, int N, int nrows) {
  GemmP g{};
  g.A = A; g.lda = lda; g.B = dz; g.ldb = ldz;
  g.C = W.g; g.ldc = W.ld; g.M = M; g.N = N; g.K = nrows;
  g.epi.kind = EPI_STORE;
  return run_gemm(h, T_DIS_GW, T_RED_DIS_GW, g, true, true);
}

// One step of generator `which` (0: G, 1: G') on the batch's users, Nu planes (G only) and policy items (device arrays); loss -> *loss_dev
int caae_g_step(ganmf_handle* h, int which, const int* users_dev, const unsigned* nu_dev, const int* items_dev, float* loss_dev) {
  CaaeState& c = h->ca;
  ProfileMlp& gn = c.gen[which];
  const int N = h->N, nb = c.Bm;
  const float pc = (which == 0 ? c.lmbda : 1.0f) / ((float)nb * (float)c.n_s), ac = which == 0 ? 1.0f - c.lmbda : 0.f;
  const std::vector<Tensor*> mine = gn.tensors();
  if (c.beta != 0.f) TRY(sumsq_tensors(h, mine, c.sq));
  TRY(caae_batch_forward(h, which, users_dev, c.R));
  GANMF_LAUNCH(caae_cdf_rows_kernel, dim3(nb), dim3(256), 0, h->st, c.R.get(), h->ldN, N, (float*)nullptr, h->ldN, c.lse.get());
  HIP_TRY(hipGetLastError());
  const long long nd = (long long)nb * c.n_s;
  GANMF_LAUNCH(caae_reward_kernel, dim3((int)((nd + 3) / 4)), dim3(256), 0, h->st, users_dev, items_dev, nb, c.n_s, h->Ue.p.get(), h->V.p.get(), c.bias.p.get(),
               h->k, h->ldk, which == 0 ? 1.0f : -1.0f, c.reward.get());
  HIP_TRY(hipGetLastError());
  CaaePolP pp{c.R, c.C, which == 0 ? nu_dev : (const unsigned*)nullptr, items_dev, c.reward, c.lse, c.dz, c.la, c.ae, h->ldN, N, c.words, c.n_s, pc, ac};
  GANMF_LAUNCH(caae_policy_kernel, dim3(nb), dim3(256), 0, h->st, pp);
  HIP_TRY(hipGetLastError());
  GANMF_LAUNCH(caae_g_loss_kernel, dim3(1), dim3(256), 0, h->st, c.la.get(), c.ae.get(), nb, pc, ac, c.beta != 0.f ? c.sq : (const float*)nullptr,
               (int)mine.size() * CFGAN_SQ_BLOCKS, c.beta, loss_dev);
  HIP_TRY(hipGetLastError());
  // backward, top down: every product reads the pre-step parameters; the updates follow
  TRY(mlp_backward(h, gn, c.C, c.dz, c.dh0, c.dh1, nb, [&](const float* A, int lda, const float* dz, int ldz, Tensor& W, int Mw, int Nw) {
    return caae_wgrad(h, A, lda, dz, ldz, W, Mw, Nw, nb);
  }));
  for (Tensor* t : mine) {
    const long long n4 = (long long)(t->padded() / 4);
    GANMF_LAUNCH(caae_sgd_kernel, dim3(caae_grid(n4)), dim3(256), 0, h->st, t->p.get(), t->g, n4, c.lr, c.beta);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

