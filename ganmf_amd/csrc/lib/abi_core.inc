// abi_core.inc -- C ABI: version, CRC-32C, create / destroy, communicators, URM upload, tensors, Adam powers
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

int ganmf_abi_version(void) { return GANMF_ABI_VERSION; }
const char* ganmf_last_error(void) { return g_err.c_str(); }

// CRC-32C, slicing-by-8 (reflected polynomial 0x82F63B78); host only.
static uint32_t g_crc_tab[8][256];
static std::once_flag g_crc_once;
static void crc_init() {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
    g_crc_tab[0][i] = c;
  }
  for (uint32_t i = 0; i < 256; ++i)
    for (int t = 1; t < 8; ++t) g_crc_tab[t][i] = (g_crc_tab[t - 1][i] >> 8) ^ g_crc_tab[0][g_crc_tab[t - 1][i] & 0xff];
}
uint32_t ganmf_crc32c(uint32_t crc, const void* data, uint64_t n) {
  std::call_once(g_crc_once, crc_init);
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint32_t c = ~crc;
  while (n >= 8) {
    uint64_t w;
    memcpy(&w, p, 8);
    w ^= c;
    c = g_crc_tab[7][w & 0xff] ^ g_crc_tab[6][(w >> 8) & 0xff] ^ g_crc_tab[5][(w >> 16) & 0xff] ^
        g_crc_tab[4][(w >> 24) & 0xff] ^ g_crc_tab[3][(w >> 32) & 0xff] ^ g_crc_tab[2][(w >> 40) & 0xff] ^
        g_crc_tab[1][(w >> 48) & 0xff] ^ g_crc_tab[0][(w >> 56) & 0xff];
    p += 8; n -= 8;
  }
  while (n--) c = (c >> 8) ^ g_crc_tab[0][(c ^ *p++) & 0xff];
  return ~c;
}

int ganmf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int64_t ganmf_live_device_bytes(void) { return (int64_t)g_live_device_bytes.load(); }

static int create_impl(const ganmf_cfg* cfg, ganmf_handle* h);

int ganmf_create(const ganmf_cfg* cfg, ganmf_handle** out) {
  if (!cfg || !out) return fail(-1, "ganmf_create: null argument");
  if (cfg->abi_version != GANMF_ABI_VERSION) return fail(-1, "ganmf_create: ABI version %d != %d", cfg->abi_version, GANMF_ABI_VERSION);
  if (cfg->model != GANMF_MODEL_GANMF && cfg->model != GANMF_MODEL_DISGANMF && cfg->model != GANMF_MODEL_MF && cfg->model != GANMF_MODEL_ITEMSIM && cfg->model != GANMF_MODEL_CFGAN && cfg->model != GANMF_MODEL_CAAE) return fail(-1, "ganmf_create: unknown model %d", cfg->model);
  if (cfg->model == GANMF_MODEL_DISGANMF && (cfg->d_layers < 1 || cfg->d_layers > 16 || cfg->d_act < 0 || cfg->d_act > 3))
    return fail(-1, "ganmf_create: DisGANMF needs 1 <= d_layers <= 16 and a known activation");
  if (cfg->model == GANMF_MODEL_CFGAN) {
    if (cfg->d_layers < 1 || cfg->d_layers > 16 || cfg->d_act < 0 || cfg->d_act > 3)
      return fail(-1, "ganmf_create: CFGAN needs 1 <= d_layers <= 16 and a known activation");
    if (cfg->world_size > 1) return fail(-1, "ganmf_create: GANMF_MODEL_CFGAN is single-GPU (world_size %d)", cfg->world_size);
    if (cfg->flags & (GANMF_FLAG_MFMA_BF16 | GANMF_FLAG_MFMA_F16))
      return fail(-1, "ganmf_create: GANMF_MODEL_CFGAN runs the fp32-accurate products only (the bf16 / fp16 MFMA flags are refused)");
    if (cfg->num_items > (1LL << 29)) return fail(-1, "ganmf_create: CFGAN's discriminator input is 2 x num_items wide: dimension too large");
  }
  if (cfg->model == GANMF_MODEL_CAAE) {
    if (cfg->world_size > 1) return fail(-1, "ganmf_create: GANMF_MODEL_CAAE is single-GPU (world_size %d)", cfg->world_size);
    if (cfg->flags & (GANMF_FLAG_MFMA_BF16 | GANMF_FLAG_MFMA_F16))
      return fail(-1, "ganmf_create: GANMF_MODEL_CAAE runs the fp32-accurate products only (the bf16 / fp16 MFMA flags are refused)");
    if (cfg->num_factors > GANMF_CAAE_MAX_FACTORS) return fail(-1, "ganmf_create: GANMF_MODEL_CAAE holds at most %d factors", GANMF_CAAE_MAX_FACTORS);
  }
  if (cfg->num_users < 1 || cfg->num_items < 1 || cfg->num_factors < 1 || cfg->emb_dim < 1 || cfg->batch_size < 1)
    return fail(-1, "ganmf_create: non-positive dimension");
  if (cfg->num_users > (1LL << 30) || cfg->num_items > (1LL << 30)) return fail(-1, "ganmf_create: dimension too large");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(-2, "ganmf_create: no HIP device (the HIP path is the only path; there is no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(-1, "ganmf_create: device %d out of range [0,%d)", cfg->device, ndev);
  HIP_TRY(hipSetDevice(cfg->device));
  ganmf_handle* h = new ganmf_handle();
  const int rc = create_impl(cfg, h);
  if (rc != 0) {
    // a failed create owns nothing afterwards: every buffer / stream / event allocated so far is released (destroy
    // tolerates null members) and a sticky hipErrorOutOfMemory is cleared, so the caller (tune.py maps MemoryError to
    // fitness 0 and keeps running trials in the same process) neither leaks HBM nor sees a spurious error later
    const std::string msg = g_err;
    ganmf_destroy(h);
    (void)hipGetLastError();
    g_err = msg;
    *out = nullptr;
    return rc;
  }
  *out = h;
  return 0;
}

static int create_impl(const ganmf_cfg* cfg, ganmf_handle* h) {
  h->cfg = *cfg;
  h->dev = cfg->device;
  h->U = (int)cfg->num_users; h->N = (int)cfg->num_items; h->k = cfg->num_factors; h->e = cfg->emb_dim;
  h->B = (int)std::min<int64_t>(cfg->batch_size, cfg->num_users);
  h->ldN = round_up(h->N + 2, LD_ALIGN); h->ldk = round_up(h->k + 1, LD_ALIGN); h->lde = round_up(h->e + 1, LD_ALIGN);
  h->tune.tile = tune_env_int("tile", 0);
  if (h->tune.tile != 0 && h->tune.tile != 64 && h->tune.tile != 128) h->tune.tile = 0;
  h->tune.ring = tune_env_int("ring", 0);
  if (h->tune.ring != 0 && h->tune.ring != 2 && h->tune.ring != 3 && h->tune.ring != 4) h->tune.ring = 0;
  h->tune.nsplit = std::max(0, tune_env_int("nsplit", 0));
  h->tune.mode = env_mfma_mode((cfg->flags & GANMF_FLAG_MFMA_F16) ? MFMA_F16 : (cfg->flags & GANMF_FLAG_MFMA_BF16) ? MFMA_BF16 : (cfg->flags & GANMF_FLAG_MFMA_F32) ? MFMA_F32 : MFMA_DEFAULT);
  h->tune.persist = tune_env_int("persist", -1);
  if (h->tune.persist > 1) h->tune.persist = 1;
  h->tune.kg = tune_env_int("kg", 0);
  h->tune.tile_order = tune_env_int("tile_order", 0);
  h->pass_stage = tune_env_int("pass_stage", 1) != 0;
  h->skinny = tune_env_int("skinny", 1) != 0;
  h->skinny_n = h->skinny && tune_env_int("skinny_n", 1) != 0;
  h->lazy_rows = tune_env_int("lazy_rows", 1) != 0;
  // (a library built by another hipcc than the tested one -- make ALLOW_UNTESTED_HIPCC=1 -- keeps the kernels with the inline-asm operand
  // prefetch off unless the environment asks for them: csrc/Makefile)
#ifdef GANMF_ASM_PREFETCH_UNTESTED
  constexpr int kAsmPrefetchDefault = 0;
#else
  constexpr int kAsmPrefetchDefault = 1;
#endif
  h->bf16w = tune_env_int("bf16w", kAsmPrefetchDefault);
  h->wgrad_xb = std::max(0, tune_env_int("wgrad_xb", 16));
  h->g_rows_staged = std::max(0, std::min(2, tune_env_int("g_rows_staged", 1)));
  h->adam_touch = tune_env_int("adam_touch", 1) != 0 ? 1 : 0;
  h->gram_arith = tune_env_int("gram", 1) == 0 ? 0 : 1;
  if (h->tune.kg != 0 && h->tune.kg != 1 && h->tune.kg != 2 && h->tune.kg != 4) h->tune.kg = 0;
  h->debug_plan = env_int("GANMF_DEBUG_PLAN", 0) != 0;
  HIP_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&h->st2, hipStreamNonBlocking));
  // lane events order two streams of THIS device only: no system-scope fence when they are recorded (the cache write-back /
  // invalidate a host-visible event performs showed as ~7 us of idle main lane per fork or join in the data-parallel step's
  // rocprofv3 timeline, profiles/r03_dp_timeline.md; kernel boundaries keep their device-scope release / acquire)
  // With more than one rank the events also order RCCL's peer writes (all-gather results land in We / Wd / V from other GPUs)
  // before the main-lane kernels that read them: the fence-free form has only ever run on one GPU, so world_size > 1 keeps the
  // system-scope fence until a multi-GPU bitwise-replica run has passed without it (GANMF_LANE_EVENT_FENCE = 0 / 1 overrides).
  const bool lane_fence = env_int("GANMF_LANE_EVENT_FENCE", cfg->world_size > 1 ? 1 : 0) != 0;
  const unsigned lane_flags = lane_fence ? hipEventDisableTiming : (hipEventDisableTiming | hipEventDisableSystemFence);
  HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, lane_flags));
  HIP_TRY(hipEventCreateWithFlags(&h->ev_join, lane_flags));
  HIP_TRY(hipEventCreateWithFlags(&h->ev_mid, lane_flags));
  HIP_TRY(hipEventCreateWithFlags(&h->ev_we, lane_flags));
  HIP_TRY(hipEventCreateWithFlags(&h->ev_wd, lane_flags));
  // GANMF_MULTI: bits 0-4 the combined launches (gemm_multi.hpp), bit 5 (32) gUb's split-K slabs summed by adam_rows_kernel,
  // bit 6 (64) DisGANMF: the hidden layers' TF-Adam in the epilogue of their gradient GEMMs
  const int multi_env = env_int("GANMF_MULTI", 127);
  h->multi = multi_env & 31;
  h->defer_gub = (multi_env & 32) != 0;
  h->dis_fuse_hidden = (multi_env & 64) != 0;
  h->x3kg = env_int("GANMF_X3KG", kAsmPrefetchDefault ? 7 : 0);      // +10 % steps/s at the ML-1M shape (profiles/r03_gemm_stamps.md)
  h->force_coll = env_int("GANMF_FORCE_COLLECTIVES", 0) != 0;
  h->score_presplit = env_int("GANMF_SCORE_PRESPLIT", 1) != 0;
  const int U = h->U, N = h->N, k = h->k, e = h->e, B = h->B;
  const bool dis = cfg->model == GANMF_MODEL_DISGANMF;
  const bool sim = cfg->model == GANMF_MODEL_ITEMSIM;      // a weighted URM and an item similarity matrix: no tensor at all
  const bool cfgan = cfg->model == GANMF_MODEL_CFGAN;      // two MLPs: the discriminator here, the generator and the work buffers by ganmf_cfgan_init
  const bool caae = cfg->model == GANMF_MODEL_CAAE;        // the factor tensors are its discriminator's; everything else by ganmf_caae_init
  const bool mf = cfg->model == GANMF_MODEL_MF || sim || caae;      // factors only (or not even those): no discriminator, no minibatch buffers
  if (caae && low_precision(h)) return fail(-1, "ganmf_create: GANMF_MODEL_CAAE runs the fp32-accurate products only (GANMF_MFMA asks for bf16 / f16)");
  // parameters; D gradients contiguous for a single all-reduce
  const int world = std::max(1, (int)cfg->world_size);
  if (!sim && !cfgan) {
    TRY(alloc_tensor(h->Ue, U, k, false, 1));      // rows of U belong to their rank: never communicated
    TRY(alloc_tensor(h->V, N, k, true, world));
    TRY(h->V_alt.alloc(h->V.cap, true));
  }
  if (mf) {
  } else if (cfgan) {
    TRY(cfgan_create(h));
  } else if (!dis) {
    TRY(alloc_tensor(h->We, N + 1, e, false, world));   // We_ext: row N = encoder bias
    TRY(alloc_tensor(h->Wd, e + 1, N, false, world, h->ldN));   // Wd_ext: row e = decoder bias; shares the leading dimension of the [.., N] work buffers
    h->gD_elems = h->We.cap + h->Wd.cap;
    TRY(h->gD.alloc(h->gD_elems, true));
    h->We.g = h->gD;
    h->Wd.g = h->We.g + h->We.cap;
  } else {
    h->L = cfg->d_layers; h->act = cfg->d_act;
    h->Wl.resize(h->L);
    h->dis_fused.assign(h->L, 0);
    h->dis_regn.assign(h->L, ADAM_GRID);
    h->gD_elems = 0;
    for (int l = 0; l < h->L; ++l) {
      TRY(alloc_tensor(h->Wl[l], l == 0 ? N + 2 : e + 1, e, false, world));
      h->gD_elems += h->Wl[l].cap;
    }
    TRY(alloc_tensor(h->Wo, 1, e + 1, false, world));
    h->gD_elems += h->Wo.cap;
    TRY(h->gD.alloc(h->gD_elems, true));
    float* gp = h->gD;
    for (int l = 0; l < h->L; ++l) { h->Wl[l].g = gp; gp += h->Wl[l].cap; }
    h->Wo.g = gp;
  }
  TRY(h->zero_page.alloc(2048 + 64, true));   // 8 KiB: one 32-byte line per lane of a workgroup
  TRY(h->perm.alloc((size_t)3 * U, true));
  h->pos = h->perm + U;
  h->pos_step = h->perm + 2 * (size_t)U;
  if (!mf && !cfgan) {      // minibatch work buffers of the adversarial step
    TRY(h->XF_own.alloc((size_t)2 * B * h->ldN, true));
    h->XF = h->XF_own;
    TRY(h->Ub_own.alloc((size_t)B * h->ldk, true));
    h->Ub = h->Ub_own;
    TRY(h->dF.alloc((size_t)B * h->ldN, true));
    TRY(h->gUb_own.alloc((size_t)B * h->ldk, true));
    h->gUb = h->gUb_own;
    // bias-folding ones columns: XF[:, N] = 1 (and E[:, e] = 1 / a_l[:, e] = 1) for every row; epilogues never store there
    std::vector<float> ones((size_t)2 * B, 1.0f);
    HIP_TRY(hipMemcpy2D(h->XF + N, (size_t)h->ldN * 4, ones.data(), 4, 4, (size_t)2 * B, hipMemcpyHostToDevice));
    if (!dis) {
      TRY(h->E.alloc((size_t)2 * B * h->lde, true));
      TRY(h->Es.alloc((size_t)2 * B * h->lde, true));
      TRY(h->Dl.alloc((size_t)2 * B * h->ldN, true));
      TRY(h->dE.alloc((size_t)2 * B * h->lde, true));
      HIP_TRY(hipMemcpy2D(h->E + e, (size_t)h->lde * 4, ones.data(), 4, 4, (size_t)2 * B, hipMemcpyHostToDevice));
    } else {
      h->Al.resize(h->L);
      for (int l = 0; l < h->L; ++l) {
        TRY(h->Al[l].alloc((size_t)2 * B * h->lde, true));
        HIP_TRY(hipMemcpy2D(h->Al[l] + e, (size_t)h->lde * 4, ones.data(), 4, 4, (size_t)2 * B, hipMemcpyHostToDevice));
      }
      TRY(h->dz0.alloc((size_t)2 * B * h->lde, true));
      TRY(h->dz1.alloc((size_t)2 * B * h->lde, true));
      TRY(h->dlogit.alloc((size_t)2 * B, true));
    }
  }
  TRY(h->rs.alloc((size_t)2 * B, true));
  h->tab_cap = (int)(U / std::max(B, 1)) + 2;
  TRY(h->scal.alloc((size_t)S_TAB + 4 * (size_t)h->tab_cap, true));
  TRY(h->sqp.alloc((size_t)2 * std::max(GEMM_RED_GRID, ((B + 63) / 64) * ((N + 63) / 64)) + 16, true));
  {
    auto t64 = [](int a, int b) { return ((a + 63) / 64) * ((b + 63) / 64); };
    h->reg_cap = std::max({ADAM_GRID, (int)GEMM_RED_GRID, t64(N + 2, e), t64(e + 1, N), t64(N, k), t64(B, N), t64(B, e)});
    h->reg_cap = round_up(h->reg_cap + (e + 63) / 64, 64);      // + the float(uid) row's partials (dis_uid_grad_kernel)
    // DisGANMF: a segment also holds the per-row cross-entropies of a batch half or the feature-matching partials
    h->dis_cap = round_up(std::max({h->reg_cap, B, dis_dz_top_blocks(e) + 1}), 64);
  }
  const float pw[4] = {ADAM_B1, ADAM_B2, ADAM_B1, ADAM_B2};
  HIP_TRY(hipMemcpy(h->scal, pw, sizeof pw, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

int ganmf_destroy(ganmf_handle* h) {
  if (!h) return 0;
  hipSetDevice(h->dev);
  if (h->st) hipStreamSynchronize(h->st);
  if (h->has_comm && !h->local && !h->comm_aborted) ncclCommDestroy(h->comm);      // (ncclCommAbort has freed an aborted one)
  if (h->local) {
    std::lock_guard<std::mutex> lk(h->local->mu);
    h->local->failed = true;            // a group does not outlive any of its members
    h->local->cv.notify_all();
  }
  for (auto& r : h->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  if (h->st2) hipStreamSynchronize(h->st2);
  if (h->ev_fork) hipEventDestroy(h->ev_fork);
  if (h->ev_join) hipEventDestroy(h->ev_join);
  if (h->ev_mid) hipEventDestroy(h->ev_mid);
  if (h->ev_t0) hipEventDestroy(h->ev_t0);
  if (h->ev_t1) hipEventDestroy(h->ev_t1);
  if (h->ev_we) hipEventDestroy(h->ev_we);
  if (h->ev_wd) hipEventDestroy(h->ev_wd);
  if (h->st2) hipStreamDestroy(h->st2);
  if (h->st) hipStreamDestroy(h->st);
  delete h;      // the members free what they own: every stream was drained above
  return 0;
}

int ganmf_comm_unique_id(uint8_t out128[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(out128, &id, 128);
  return 0;
}

int ganmf_comm_init_local(ganmf_handle* h, int32_t group_id) {
  if (!h) return fail(-1, "null handle");
  TRY(not_cfgan(h, "ganmf_comm_init_local"));
  if (h->has_comm) return fail(-1, "ganmf_comm_init_local: handle already has a communicator");
  const int world = h->cfg.world_size, rank = h->cfg.rank;
  if (world < 1 || world > LOCAL_MAX_WORLD || rank < 0 || rank >= world)
    return fail(-1, "ganmf_comm_init_local: world_size %d / rank %d out of range (max %d)", world, rank, LOCAL_MAX_WORLD);
  std::lock_guard<std::mutex> lk(g_local_mu);
  std::shared_ptr<LocalGroup>& slot = g_local_groups[group_id];
  if (!slot || slot->joined == slot->world || slot->failed) {      // first member of a new group with this id
    slot = std::make_shared<LocalGroup>();
    slot->world = world; slot->dev = h->dev;
  }
  if (slot->world != world || slot->dev != h->dev)
    return fail(-1, "ganmf_comm_init_local: group %d is for world_size %d on device %d", group_id, slot->world, slot->dev);
  ++slot->joined;
  h->local = slot;
  h->has_comm = true;
  return 0;
}

int ganmf_comm_init(ganmf_handle* h, const uint8_t id128[128]) {
  if (!h) return fail(-1, "null handle");
  TRY(not_cfgan(h, "ganmf_comm_init"));
  HIP_TRY(hipSetDevice(h->dev));
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  NCCL_TRY(ncclCommInitRank(&h->comm, h->cfg.world_size, id, h->cfg.rank));
  h->has_comm = true;
  return 0;
}

int ganmf_comm_info(ganmf_handle* h, int32_t* world_size, int32_t* rank) {
  if (!h || !world_size || !rank) return fail(-1, "ganmf_comm_info: null argument");
  *world_size = 0; *rank = -1;
  if (!h->has_comm) return 0;
  if (h->local) { *world_size = h->local->world; *rank = h->cfg.rank; return 0; }
  int n = 0, r = -1;
  std::lock_guard<std::mutex> comm_lk(h->comm_mu);
  if (h->comm_aborted.load(std::memory_order_acquire)) return fail(-3, "ganmf_comm_info: communicator aborted (ganmf_comm_abort)");
  NCCL_TRY(ncclCommCount(h->comm, &n));
  NCCL_TRY(ncclCommUserRank(h->comm, &r));
  *world_size = n; *rank = r;
  return 0;
}

int ganmf_comm_abort(ganmf_handle* h) {
  if (!h) return fail(-1, "ganmf_comm_abort: null handle");
  if (!h->has_comm) return 0;
  if (h->local) {      // (only the group's own mutex-protected state is touched: safe beside a training call of the handle's thread)
    std::lock_guard<std::mutex> lk(h->local->mu);
    h->local->failed = true;
    h->local->cv.notify_all();
    return 0;
  }
  // flag first (the handle's thread stops enqueueing at its next wrapper), then the lock: an enqueue in flight returns before the free
  if (!h->comm_aborted.exchange(true, std::memory_order_acq_rel)) {
    std::lock_guard<std::mutex> comm_lk(h->comm_mu);
    NCCL_TRY(ncclCommAbort(h->comm));
  }
  return 0;
}

int ganmf_set_urm_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const float* data,
                      int64_t n_rows, int64_t n_cols) {
  if (!h || !indptr || ((!indices || !data) && indptr[n_rows] > 0)) return fail(-1, "ganmf_set_urm_csr: null argument");
  if (n_rows != h->U || n_cols != h->N) return fail(-1, "ganmf_set_urm_csr: shape %lldx%lld != handle %dx%d", (long long)n_rows, (long long)n_cols, h->U, h->N);
  int64_t nnz = indptr[n_rows];
  if (indptr[0] != 0 || nnz < 0) return fail(-1, "ganmf_set_urm_csr: bad indptr");
  for (int64_t r = 0; r < n_rows; ++r)
    if (indptr[r + 1] < indptr[r]) return fail(-1, "ganmf_set_urm_csr: indptr not monotone at row %lld", (long long)r);
  for (int64_t j = 0; j < nnz; ++j)
    if (indices[j] < 0 || indices[j] >= n_cols) return fail(-1, "ganmf_set_urm_csr: column index %d out of range at %lld", indices[j], (long long)j);
  // Canonical form, as scipy's sum_duplicates() + sort_indices() leave it: every row's columns strictly ascending, the entries of a
  // repeated (row, column) summed in stored order, explicit zeros kept.  The reference feeds URM_train[uids].toarray() -- which sums
  // duplicates -- whatever form the matrix has; the device paths need the canonical one (densify_rows scatters one store per entry,
  // csr_quad binary-searches a row).  A canonical input is uploaded as it is.
  std::vector<int64_t> c_indptr;
  std::vector<int> c_indices;
  std::vector<float> c_data;
  bool canonical = true;
  for (int64_t r = 0; r < n_rows && canonical; ++r)
    for (int64_t j = indptr[r] + 1; j < indptr[r + 1]; ++j)
      if (indices[j] <= indices[j - 1]) { canonical = false; break; }
  if (!canonical) {
    c_indptr.assign((size_t)n_rows + 1, 0);
    c_indices.reserve((size_t)nnz);
    c_data.reserve((size_t)nnz);
    std::vector<int64_t> order;
    for (int64_t r = 0; r < n_rows; ++r) {
      order.resize((size_t)(indptr[r + 1] - indptr[r]));
      for (size_t i = 0; i < order.size(); ++i) order[i] = indptr[r] + (int64_t)i;
      std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return indices[a] < indices[b]; });
      for (size_t i = 0; i < order.size(); ++i) {
        const int64_t j = order[i];
        if (i > 0 && indices[j] == c_indices.back()) c_data.back() += data[j];
        else { c_indices.push_back(indices[j]); c_data.push_back(data[j]); }
      }
      c_indptr[(size_t)r + 1] = (int64_t)c_indices.size();
    }
    indptr = c_indptr.data();
    indices = c_indices.data();
    data = c_data.data();
    nnz = (int64_t)c_indices.size();
  }
  HIP_TRY(hipSetDevice(h->dev));
  // what is held goes first, the facts beside it are set last: a failure anywhere leaves "no URM" (and no CSC twin)
  h->has_urm = false; h->sparse_g = false; h->sparse_d = false;
  h->data.reset(); h->csc.drop(); h->csc_val.reset();
  TRY(h->urm.upload(indptr, indices, n_rows, n_cols));
  TRY(h->urm.upload_values(h->data, data));
  h->ca.iu_src = nullptr;      // CAAE: the users of the stored interactions are formed again from this matrix (caae_prepare)
  // SURVEY 8(f)-3: below 0.5 % density (LastFM: 0.22 %) the generator step reads the real rows as CSR (GANMF only;
  // DisGANMF feeds the rows themselves to its discriminator).  GANMF_SPARSE = 0 / 1 overrides.
  const double density = (double)nnz / ((double)n_rows * (double)n_cols);
  const int force = env_int("GANMF_SPARSE", -1);
  h->sparse_g = h->cfg.model == GANMF_MODEL_GANMF && (force >= 0 ? force != 0 : density < 0.005);
  // The discriminator step's sparse path trades 4.B.N.e dense FLOPs (real half of the encode GEMM and of the encoder-gradient
  // GEMM) and the [B, N] row expansion for a CSR row-sum, a CSR lookup per residual element and a CSC walk per gradient element:
  // it pays once those FLOPs are worth more than the few microseconds the lookups add to two epilogues (LastFM at the reference's
  // defaults, B = 32, e = 32: 0.07 GFLOP -- dense; at its tuned B = 1024, e = 398: 28.7 GFLOP of a 146 GFLOP step -- sparse).
  // GANMF_SPARSE_D = 0 / 1 overrides (GANMF_SPARSE = 0 switches both paths off).
  const int force_d = env_int("GANMF_SPARSE_D", -1);
  const double flops_saved = 4.0 * (double)h->B * (double)h->N * (double)h->e;
  h->sparse_d = h->cfg.model == GANMF_MODEL_GANMF && force != 0 &&
                (force_d >= 0 ? force_d != 0 : (density < 0.005 && flops_saved >= 2.0e9));
  if (h->debug_plan)      // (tests assert on the path the planner took, not only on the numbers it produced)
    fprintf(stderr, "[ganmf urm] set_urm_csr %lldx%lld nnz=%lld%s density %.5f -> sparse_g %d sparse_d %d\n", (long long)n_rows,
            (long long)n_cols, (long long)nnz, canonical ? "" : " (made canonical)", density, (int)h->sparse_g, (int)h->sparse_d);
  if (h->sparse_d) {      // counting sort by column; rows ascend inside a column because the CSR rows are walked in order
    std::vector<long long> colptr((size_t)n_cols + 1, 0);
    for (int64_t j = 0; j < nnz; ++j) ++colptr[(size_t)indices[j] + 1];
    for (int64_t c = 0; c < n_cols; ++c) colptr[c + 1] += colptr[c];
    std::vector<long long> fill(colptr.begin(), colptr.end() - 1);
    std::vector<int> rowidx((size_t)std::max<int64_t>(nnz, 1));
    std::vector<float> val((size_t)std::max<int64_t>(nnz, 1));
    for (int64_t r = 0; r < n_rows; ++r)
      for (int64_t j = indptr[r]; j < indptr[r + 1]; ++j) {
        const long long at = fill[indices[j]]++;
        rowidx[at] = (int)r; val[at] = data[j];
      }
    int rc = h->csc.upload(colptr.data(), rowidx.data(), n_cols, n_rows);
    if (!rc) rc = h->csc.upload_values(h->csc_val, val.data());
    if (!rc && !h->sp_rows) rc = h->sp_rows.alloc((size_t)(h->N + CSC_BIAS_PARTS) * h->lde, true);
    if (rc) { h->urm.drop(); h->data.reset(); h->csc.drop(); h->csc_val.reset(); h->sparse_g = h->sparse_d = false; return rc; }
  }
  if (!h->sparse_d) h->sp_rows.reset();      // (scratch of the sparse discriminator step only)
  h->has_urm = true;
  return 0;
}

int ganmf_tensor_shape(ganmf_handle* h, int tensor_id, int64_t* rows, int64_t* cols) {
  View v;
  if (h) TRY(needs_tensors(h, "ganmf_tensor_shape"));
  if (!h || !find_view(h, tensor_id, &v)) return fail(-1, "unknown tensor id %d", tensor_id);
  if (rows) *rows = v.rows;
  if (cols) *cols = v.cols;
  return 0;
}

static int copy_view(ganmf_handle* h, int tensor_id, int slot, float* host, int64_t n, bool to_device, const char* who) {
  View v;
  if (h) TRY(needs_tensors(h, who));
  if (!h || !host || !find_view(h, tensor_id, &v)) return fail(-1, "%s: unknown tensor id %d", who, tensor_id);
  if (n != (int64_t)v.rows * v.cols) return fail(-1, "%s: tensor %d has %lld elements, got %lld", who, tensor_id, (long long)v.rows * v.cols, (long long)n);
  // data-parallel runs keep the Adam moments of a REPLICATED tensor sharded: rank r updates slice r only (dp_update), the other
  // slices of its m / v buffers are stale.  Reading or writing them through one rank would silently give a different optimizer.
  if ((slot == GANMF_SLOT_ADAM_M || slot == GANMF_SLOT_ADAM_V) && h->has_comm && h->cfg.world_size > 1 && tensor_id != GANMF_T_USER_EMB)
    return fail(-1, "%s: the Adam moments of replicated tensor %d are sharded over the %d ranks of a data-parallel run "
                    "(each rank holds its slice only); only user_embeddings' moments are whole on their rank", who, tensor_id, h->cfg.world_size);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  for (int i = 0; i < v.nseg; ++i) {
    const Seg& sg = v.seg[i];
    float* d = slot_ptr(sg.t, slot);
    if (!d) return fail(-1, "%s: bad slot %d", who, slot);
    d += (size_t)sg.row0 * sg.t->ld + sg.col0;
    float* hp = host + (size_t)sg.host_row0 * v.cols;
    // a [e,1] view stored as one row of e floats: host pitch is the segment's own width
    const size_t hpitch = (size_t)sg.cols * 4, dpitch = (size_t)sg.t->ld * 4;
    if (to_device) HIP_TRY(hipMemcpy2D(d, dpitch, hp, hpitch, (size_t)sg.cols * 4, sg.rows, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemcpy2D(hp, hpitch, d, dpitch, (size_t)sg.cols * 4, sg.rows, hipMemcpyDeviceToHost));
  }
  return 0;
}

int ganmf_set_tensor(ganmf_handle* h, int tensor_id, int slot, const float* host, int64_t n) {
  if (h) ++h->param_version;
  return copy_view(h, tensor_id, slot, const_cast<float*>(host), n, true, "ganmf_set_tensor");
}

int ganmf_get_tensor(ganmf_handle* h, int tensor_id, int slot, float* host, int64_t n) {
  return copy_view(h, tensor_id, slot, host, n, false, "ganmf_get_tensor");
}

int ganmf_get_adam_powers(ganmf_handle* h, float out4[4]) {
  if (!h) return fail(-1, "null handle");
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  HIP_TRY(hipMemcpy(out4, h->scal, 4 * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_set_adam_powers(ganmf_handle* h, const float in4[4]) {
  if (!h) return fail(-1, "null handle");
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  HIP_TRY(hipMemcpy(h->scal, in4, 4 * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

