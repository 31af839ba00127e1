// profile_mlp.inc -- the profile MLP (ProfileMlp, handle.inc) that is CFGAN's generator and both of CAAE's: its buffers, the forward
// pass over dense rows or over rows of the URM, sum(theta^2) of a tensor list, and the backward walk
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// Every dense product goes through run_gemm under the handle's planner.

// a block [rows, ldg] of hidden outputs: zero, with the ones column at g
int mlp_hidden_block(const ProfileMlp& m, DevBuf<float>& p, size_t rows) {
  TRY(p.alloc(rows * m.ldg, true));
  std::vector<float> ones(rows, 1.0f);
  HIP_TRY(hipMemcpy2D(p + m.g, (size_t)m.ldg * 4, ones.data(), 4, 4, rows, hipMemcpyHostToDevice));
  return 0;
}

// the tensors (each owns its gradient buffer) and the hidden blocks of a training batch of `rows` rows
int mlp_alloc(ganmf_handle* h, ProfileMlp& m, int g, int Lg, int act, int out_act, int rows) {
  m.g = g; m.Lg = Lg; m.act = act; m.out_act = out_act; m.ldg = round_up(g + 1, LD_ALIGN);
  m.Gl.resize(Lg);
  for (int l = 0; l < Lg; ++l) TRY(alloc_tensor(m.Gl[l], l == 0 ? h->N + 1 : g + 1, g, true, 1));
  TRY(alloc_tensor(m.Go, g + 1, h->N, true, 1, h->ldN));
  m.Hl.clear();
  m.Hl.resize(Lg);
  for (int l = 0; l < Lg; ++l) TRY(mlp_hidden_block(m, m.Hl[l], (size_t)rows));
  return 0;
}

// the scratch blocks for `rows` rows
int mlp_scratch(ganmf_handle* h, ProfileMlp& m, size_t rows) {
  if (rows <= m.sc_rows) return 0;
  HIP_TRY(hipStreamSynchronize(h->st));
  m.sc_C.reset(); m.sc_H0.reset(); m.sc_H1.reset(); m.sc_F.reset();
  m.sc_rows = 0;
  TRY(m.sc_C.alloc(rows * h->ldN, true));
  TRY(mlp_hidden_block(m, m.sc_H0, rows));
  TRY(mlp_hidden_block(m, m.sc_H1, rows));
  TRY(m.sc_F.alloc(rows * h->ldN, true));
  m.sc_rows = rows;
  return 0;
}

// out[nb, ldo] = M(X) for the nb dense rows X [nb, ldN] (ones column at N); hidden outputs into H[l] [nb, ldg] (ones column at g)
int mlp_forward(ganmf_handle* h, const ProfileMlp& m, const float* X, int nb, float* const* H, float* out, int ldo) {
  for (int l = 0; l < m.Lg; ++l) {      // h_{l+1} = act([h_l | 1] . Gl_ext)
    GemmP g{};
    g.A = l == 0 ? X : H[l - 1]; g.lda = l == 0 ? h->ldN : m.ldg;
    g.B = m.Gl[l].p; g.ldb = m.ldg;
    g.C = H[l]; g.ldc = m.ldg; g.M = nb; g.N = m.g; g.K = l == 0 ? h->N + 1 : m.g + 1;
    g.epi.kind = EPI_ACT; g.epi.act = m.act;
    TRY(run_gemm(h, T_DIS_FWD, T_RED_DIS_FWD, g, false, true));
  }
  GemmP g{};      // out = [h | 1] . Go_ext
  g.A = H[m.Lg - 1]; g.lda = m.ldg; g.B = m.Go.p; g.ldb = h->ldN;
  g.C = out; g.ldc = ldo; g.M = nb; g.N = h->N; g.K = m.g + 1; g.epi.kind = EPI_STORE;
  if (m.out_act >= 0) { g.epi.kind = EPI_ACT; g.epi.act = m.out_act; }
  return run_gemm(h, T_GEMM_GEN, T_RED_GEN, g, false, true);
}

// out[i, :] = M(profile of row ids[i]) for n rows of the URM (ids_dev == nullptr: rows row0 ..).  C != nullptr: a training batch -- the
// dense profiles into C [n, ldN], the hidden outputs into the model's own blocks Hl; else through the model's scratch blocks
int mlp_forward_rows(ganmf_handle* h, ProfileMlp& m, const int* ids_dev, int row0, int n, float* out, int ldo, float* C = nullptr) {
  std::vector<float*> scratch(m.Hl.begin(), m.Hl.end());      // the hidden blocks as plain pointers
  if (!C) {
    scratch.clear();
    TRY(mlp_scratch(h, m, (size_t)n));
    C = m.sc_C;
    for (int l = 0; l < m.Lg; ++l) scratch.push_back((l & 1) ? m.sc_H1 : m.sc_H0);
  }
  GANMF_LAUNCH(cfgan_densify_kernel, dim3(n), dim3(256), 0, h->st, h->urm.indptr.get(), h->urm.indices.get(), h->data.get(), ids_dev, row0, h->N, C, h->ldN);
  HIP_TRY(hipGetLastError());
  return mlp_forward(h, m, C, n, scratch.data(), out, ldo);
}

// sq[t * CFGAN_SQ_BLOCKS ..] = the block partials of sum(theta^2) of tensor t
int sumsq_tensors(ganmf_handle* h, const std::vector<Tensor*>& ts, float* sq) {
  for (size_t t = 0; t < ts.size(); ++t)
    GANMF_LAUNCH(cfgan_sumsq_kernel, dim3(CFGAN_SQ_BLOCKS), dim3(256), 0, h->st, ts[t]->p.get(), (long long)(ts[t]->padded() / 4), sq + t * CFGAN_SQ_BLOCKS);
  HIP_TRY(hipGetLastError());
  return 0;
}

// dst = (src . W[0:n_out]^T) * act'(aux): one layer of a backward pass over nrows rows
int mlp_bwd(ganmf_handle* h, const float* src, int lds, const float* W, int ldw, float* dst, int ldd, int nrows, int n_out, int K,
            int act, const float* aux, int ldaux) {
  GemmP g{};
  g.A = src; g.lda = lds; g.B = W; g.ldb = ldw;
  g.C = dst; g.ldc = ldd; g.M = nrows; g.N = n_out; g.K = K;
  g.epi.kind = aux ? EPI_MUL_ACTGRAD : EPI_STORE; g.epi.act = act;
  g.epi.aux = aux; g.epi.ldaux = ldaux;
  return run_gemm(h, T_DIS_BWD, T_RED_DIS_BWD, g, false, false);
}

// The backward pass of a training batch, top down: X [nb, ldN] the dense rows its forward pass read, dout [nb, ldN] the gradient at the
// linear output, dh0 / dh1 [nb, ldg] the hidden gradients (the layers alternate).  wgrad(A, lda, dz, ldz, W, M, N) is the model's
// weight-gradient product W <- A_ext^T . dz; in every layer the product that reads W_l runs in front of it.
template <class WGrad>
int mlp_backward(ganmf_handle* h, ProfileMlp& m, const float* X, const float* dout, float* dh0, float* dh1, int nb, WGrad wgrad) {
  const int N = h->N, g = m.g, Lg = m.Lg;
  float* cur = dh0;
  float* nxt = dh1;
  TRY(mlp_bwd(h, dout, h->ldN, m.Go.p, h->ldN, cur, m.ldg, nb, g, N, m.act, m.Hl[Lg - 1], m.ldg));
  TRY(wgrad(m.Hl[Lg - 1], m.ldg, dout, h->ldN, m.Go, g + 1, N));
  for (int l = Lg - 1; l >= 0; --l) {
    if (l > 0) TRY(mlp_bwd(h, cur, m.ldg, m.Gl[l].p, m.ldg, nxt, m.ldg, nb, g, g, m.act, m.Hl[l - 1], m.ldg));
    TRY(wgrad(l == 0 ? X : m.Hl[l - 1], l == 0 ? h->ldN : m.ldg, cur, m.ldg, m.Gl[l], l == 0 ? N + 1 : g + 1, g));
    if (l > 0) std::swap(cur, nxt);
  }
  return 0;
}

