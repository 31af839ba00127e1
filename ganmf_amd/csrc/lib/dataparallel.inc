// dataparallel.inc -- SURVEY 8(e): communicators (RCCL / loopback), reduce-scatter / all-gather, the side lane's forks and joins, Adam on a rank's slice
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// ---- in-process loopback communicator ---------------------------------------------------------------
// Several handles of ONE process (driven by one host thread each) on the same device form a group; an all-reduce
// is a rendezvous: every member drains the stream its buffer is produced on, the last to arrive sums the buffers in
// rank order (deterministic) into every member's buffer and releases the others.  It exists so that the
// data-parallel arithmetic (global-batch scales, the two-float exchange before the hinge, ranks that run out of
// rows) can be exercised with world_size > 1 on a single GPU; multi-GPU runs use RCCL.
static std::mutex g_local_mu;
static std::map<int, std::shared_ptr<LocalGroup>> g_local_groups;

int collective_local(ganmf_handle* h, float* buf, size_t count, hipStream_t st, int op) {
  LocalGroup& g = *h->local;
  HIP_TRY(hipStreamSynchronize(st));                    // this member's contribution is complete
  std::unique_lock<std::mutex> lk(g.mu);
  if (g.failed) return fail(-3, "local communicator: a peer failed");
  if (g.arrived == 0) { g.count = count; g.op = op; }
  else if (g.count != count || g.op != op) { g.failed = true; g.cv.notify_all(); return fail(-3, "local communicator: members disagree on the collective"); }
  g.bufs.p[h->cfg.rank] = buf;
  if (++g.arrived == g.world) {
    const int grid = (int)std::min<size_t>(1024, (count + 255) / 256);
    GANMF_LAUNCH(local_collective_kernel, dim3(std::max(grid, 1)), dim3(256), 0, st, g.bufs, g.world, count, op);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    g.arrived = 0;
    ++g.generation;
    if (e != hipSuccess) g.failed = true;
    g.cv.notify_all();
    if (e != hipSuccess) return fail(-2, "local communicator: %s", hipGetErrorString(e));
    return 0;
  }
  const long long gen = g.generation;
  if (!g.cv.wait_for(lk, std::chrono::seconds(120), [&] { return g.generation != gen || g.failed; })) {
    g.failed = true;
    g.cv.notify_all();
    return fail(-3, "local communicator: timed out waiting for %d peer(s)", g.world - g.arrived);
  }
  return g.failed ? fail(-3, "local communicator: a peer failed") : 0;
}

// every RCCL call of the handle's thread goes through this: no enqueue on a communicator ganmf_comm_abort has freed (or is freeing)
#define COMM_LOCKED_OR_FAIL(h)                                   \
  std::lock_guard<std::mutex> comm_lk((h)->comm_mu);             \
  if ((h)->comm_aborted.load(std::memory_order_acquire)) return fail(-3, "communicator aborted (ganmf_comm_abort): the handle can only be destroyed")

int allreduce(ganmf_handle* h, float* buf, size_t count, int lane = 0) {
  if (!h->has_comm) return 0;
  hipStream_t st = lane ? h->st2 : h->st;
  Scope s(h, T_ALLREDUCE, 0, 4.0 * count, st);
  if (h->local) return collective_local(h, buf, count, st, LOCAL_ALLREDUCE);
  COMM_LOCKED_OR_FAIL(h);
  NCCL_TRY(ncclAllReduce(buf, buf, count, ncclFloat, ncclSum, h->comm, st));
  return 0;
}

// In place over a buffer of world equal slices: after the reduce-scatter rank r holds the sum of slice r (the other
// slices of its buffer are unspecified); the all-gather fills every slice from its owner.
int reduce_scatter(ganmf_handle* h, float* buf, size_t total, int lane, int tag = T_ALLREDUCE) {
  if (h->cfg.world_size == 1 && !h->force_coll) return 0;     // one slice, already in place
  hipStream_t st = lane ? h->st2 : h->st;
  const size_t slice = total / (size_t)h->cfg.world_size;
  Scope s(h, tag, 0, 4.0 * total, st);
  if (h->local) return collective_local(h, buf, total, st, LOCAL_REDUCE_SCATTER);
  COMM_LOCKED_OR_FAIL(h);
  NCCL_TRY(ncclReduceScatter(buf, buf + (size_t)h->cfg.rank * slice, slice, ncclFloat, ncclSum, h->comm, st));
  return 0;
}
int all_gather(ganmf_handle* h, float* buf, size_t total, int lane, int tag = T_ALLREDUCE) {
  if (h->cfg.world_size == 1 && !h->force_coll) return 0;
  hipStream_t st = lane ? h->st2 : h->st;
  const size_t slice = total / (size_t)h->cfg.world_size;
  Scope s(h, tag, 0, 4.0 * total, st);
  if (h->local) return collective_local(h, buf, total, st, LOCAL_ALLGATHER);
  COMM_LOCKED_OR_FAIL(h);
  NCCL_TRY(ncclAllGather(buf + (size_t)h->cfg.rank * slice, buf, slice, ncclFloat, h->comm, st));
  return 0;
}

// fork: the side lane starts after everything enqueued so far on the main lane
int lane_fork(ganmf_handle* h) {
  HIP_TRY(hipEventRecord(h->ev_fork, h->st));
  HIP_TRY(hipStreamWaitEvent(h->st2, h->ev_fork, 0));
  return 0;
}
// The same fork in two halves around the LAST main-lane launch the side lane has to wait for: fork_arm() before it (that launch
// then carries ev_fork as its completion event: no marker packet on the main lane), fork_wait() after it.  While the library's
// profiler is on (its scopes hand their own events to the launches) the plain fork is used.
// The attached event marks the FIRST launch after fork_arm(): the fork is only taken as attached when exactly one kernel was
// launched in between (a plan that adds a stand-alone reduce or an attached slab sum falls back to the marker-packet fork, which
// covers everything enqueued so far -- never a silent wait for the wrong kernel).
bool fork_arm(ganmf_handle* h) {
  if (h->prof) return false;
  launch_stop_event() = h->ev_fork;
  h->fork_armed_at = launch_count();
  return true;
}
int fork_wait(ganmf_handle* h, bool armed) {
  if (!armed) return lane_fork(h);
  const long long launched = launch_count() - h->fork_armed_at;
  if (launch_stop_event() != nullptr || launched != 1) {      // nothing, or more than one kernel, was launched in between: plain fork
    launch_stop_event() = nullptr;
    return lane_fork(h);
  }
  HIP_TRY(hipStreamWaitEvent(h->st2, h->ev_fork, 0));
  return 0;
}
// join: the main lane continues after everything enqueued so far on the side lane
int lane_join(ganmf_handle* h) {
  HIP_TRY(hipEventRecord(h->ev_join, h->st2));
  HIP_TRY(hipStreamWaitEvent(h->st, h->ev_join, 0));
  return 0;
}

// The main lane may not touch We / Wd again before the side lane's reduce-scatter / Adam / all-gather on them are done.
// dp_mark: everything enqueued on the side lane so far completes the update of the tensors in `mask`; dp_join: the main lane
// waits for the tensors in `mask` that are still pending -- the encoder before the next encode GEMM, the decoder only before the
// next decode GEMM, one encode GEMM later (the side lane is in order: the decoder's event implies the encoder's).
enum : int { PEND_WE = 1, PEND_WD = 2, PEND_ALL = 3 };
int dp_mark(ganmf_handle* h, int mask) {
  if (mask & PEND_WE) HIP_TRY(hipEventRecord(h->ev_we, h->st2));
  if (mask & PEND_WD) HIP_TRY(hipEventRecord(h->ev_wd, h->st2));
  h->side_pending |= mask;
  return 0;
}
int dp_join(ganmf_handle* h, int mask = PEND_ALL) {
  const int m = h->side_pending & mask;
  if (!m) return 0;
  // (while the profiler is on, each wait sits between two event records on the main lane: the time it blocked)
  if (m & PEND_WE) { Scope s(h, T_JOIN_WE, 0, 0); HIP_TRY(hipStreamWaitEvent(h->st, h->ev_we, 0)); }
  if (m & PEND_WD) { Scope s(h, T_JOIN_WD, 0, 0); HIP_TRY(hipStreamWaitEvent(h->st, h->ev_wd, 0)); }
  h->side_pending &= ~m;
  return 0;
}

int adam_dense(ganmf_handle* h, int tag, Tensor& t, const float* g, int alpha_idx, float reg, float* sq, int lane = 0,
               size_t off = 0, size_t count = 0) {
  if (count == 0) count = t.padded() - off;
  const long long n4 = (long long)count / 4;
  hipStream_t st = lane ? h->st2 : h->st;
  Scope s(h, tag, 0, 28.0 * count, st);
  GANMF_LAUNCH(adam_dense_kernel, dim3(ADAM_GRID), dim3(256), 0, st, t.p + off, t.m + off, t.v + off, g + off, n4, h->scal.get(),
                     alpha_idx, reg, sq);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Data-parallel update of a replicated tensor whose local gradient is complete in t.g (SURVEY 8e): reduce-scatter the
// gradient, TF-Adam on this rank's slice only (parameter and moment slices; the moments of a replicated tensor live
// sharded across the ranks), all-gather the parameter.  Same bytes on the links as an all-reduce, 1 / world of the Adam
// traffic, and every rank ends with bitwise identical parameters (each slice has exactly one writer).  The sum(theta^2)
// partials cover the slice only: the loss parts are all-reduced once per epoch.
int dp_update(ganmf_handle* h, int tag, Tensor& t, int alpha_idx, float reg, float* sq, int lane) {
  const size_t slice = t.cap / (size_t)h->cfg.world_size, off = (size_t)h->cfg.rank * slice;
  const int ctag = &t == &h->We ? T_COLL_WE : &t == &h->Wd ? T_COLL_WD : &t == &h->V ? T_COLL_V : T_ALLREDUCE;
  TRY(reduce_scatter(h, t.g, t.cap, lane, ctag));
  TRY(adam_dense(h, tag, t, t.g, alpha_idx, reg, sq, lane, off, slice));
  TRY(all_gather(h, t.p, t.cap, lane, ctag));
  return 0;
}

