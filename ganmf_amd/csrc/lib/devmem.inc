// devmem.inc -- device memory: the owning buffer DevBuf, the CSR holder DevCsr and the count of live device bytes.  The only file of
// the library that calls the HIP allocator (tests/test_devmem_host.py keeps it so, and runs this file on the host heap over a shim).
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "CSR row pointers and indices");

// bytes of device memory held by every DevBuf of the process (ganmf_live_device_bytes); pinned host staging is not counted
static std::atomic<long long> g_live_device_bytes{0};

// An owned array of T in device memory (Pinned: in pinned host memory): freed by the destructor, by reset() and by whatever replaces
// it.  Move-only; reads as a plain T* (a kernel launch deduces its arguments by value: pass get()).  cap: the elements it was asked for.
// Every allocation holds at least 16 bytes.
template <class T, bool Pinned = false>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T*() const { return p; }
  T* get() const { return p; }
  static size_t bytes_of(size_t n) { return std::max<size_t>(n * sizeof(T), 16); }

  void reset() {
    if (!p) return;
    if (Pinned) hipHostFree(p);
    else { hipFree(p); g_live_device_bytes -= (long long)bytes_of(cap); }
    p = nullptr; cap = 0;
  }
  // n elements in place of what it holds.  zeroed: filled with zero bytes and the device synchronised (the handle's streams do not
  // synchronise with the null stream); else the contents are undefined.  A failure leaves it empty.
  int alloc(size_t n, bool zeroed) {
    reset();
    const size_t bytes = bytes_of(n);
    const hipError_t e = Pinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(-2, "%s of %llu bytes failed: %s", Pinned ? "hipHostMalloc" : "hipMalloc", (unsigned long long)bytes, hipGetErrorString(e));
    }
    cap = n;
    if (!Pinned) g_live_device_bytes += (long long)bytes;
    if (zeroed) {
      hipError_t z = hipMemset(p, 0, bytes);
      if (z == hipSuccess) z = hipDeviceSynchronize();
      if (z != hipSuccess) { reset(); return fail(-2, "hipMemset of %llu bytes failed: %s", (unsigned long long)bytes, hipGetErrorString(z)); }
    }
    return 0;
  }
  // the same, not zeroed, for the entries whose failure names the bytes asked for and is cleared: the handle stays usable
  int alloc(const char* who, const char* what, size_t n) {
    reset();
    const hipError_t e = hipMalloc((void**)&p, bytes_of(n));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return fail(-2, "%s: out of memory: %s needs %llu bytes (%s)", who, what, (unsigned long long)(n * sizeof(T)), hipGetErrorString(e));
    }
    cap = n;
    g_live_device_bytes += (long long)bytes_of(n);
    return 0;
  }
  // room for `need` elements: nothing happens if they fit; else the stream is drained (enqueued work may still use the old array), the
  // old array is freed and a new one allocated.  The contents are NOT preserved.  A failure leaves it empty.
  int grow(hipStream_t st, size_t need, bool zeroed) {
    if (need <= cap) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    return alloc(need, zeroed);
  }
};
template <class T> using PinnedBuf = DevBuf<T, true>;

// A sparse matrix in CSR on the device: row pointers and column indices with their shape; the values live in a typed DevBuf beside it
// (float or double, or none).  One rule for every upload: drop first, set the shape last -- a failure anywhere leaves an empty holder
// (null pointers, rows == cols == nnz == 0), and held() is the one question "is a matrix there".  Facts a caller keeps beside the
// holder are reset by the caller in front of the upload and set behind it.
struct DevCsr {
  DevBuf<long long> indptr;
  DevBuf<int> indices;
  long long rows = 0, cols = 0, nnz = 0;
  bool held() const { return indptr.p != nullptr; }
  void drop() { indptr.reset(); indices.reset(); rows = cols = nnz = 0; }

  // who != null: allocation failures carry the named out-of-memory message (DevBuf::alloc(who, what, n))
  template <class T>
  static int alloc_array(DevBuf<T>& b, size_t n, const char* who, const char* what) { return who ? b.alloc(who, what, n) : b.alloc(n, false); }
  static int copy_in(void* dst, const void* src, size_t bytes, bool src_on_device) {
    const hipError_t e = hipMemcpy(dst, src, bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : fail(-2, "hipMemcpy of %llu bytes of a CSR matrix failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
  }
  // host_indptr [n_rows + 1] on the host; src_indices [nnz] on the host, or on the device (indices_on_device), or null: the array is
  // allocated for a kernel to fill
  int upload(const int64_t* host_indptr, const int32_t* src_indices, int64_t n_rows, int64_t n_cols, bool indices_on_device = false,
             const char* who = nullptr, const char* what = nullptr) {
    drop();
    const int64_t n = host_indptr[n_rows];
    int rc = alloc_array(indptr, (size_t)n_rows + 1, who, what);
    if (!rc) rc = alloc_array(indices, (size_t)std::max<int64_t>(n, 1), who, what);
    if (!rc) rc = copy_in(indptr.p, host_indptr, ((size_t)n_rows + 1) * sizeof(long long), false);
    if (!rc && n && src_indices) rc = copy_in(indices.p, src_indices, (size_t)n * sizeof(int), indices_on_device);
    if (rc) { drop(); return rc; }
    rows = n_rows; cols = n_cols; nnz = n;
    return 0;
  }
  int upload(const long long* host_indptr, const int32_t* src_indices, int64_t n_rows, int64_t n_cols, bool indices_on_device = false,
             const char* who = nullptr, const char* what = nullptr) {
    return upload(reinterpret_cast<const int64_t*>(host_indptr), src_indices, n_rows, n_cols, indices_on_device, who, what);
  }
  // the value array [nnz] of the held matrix into `vals` (src null: allocated only); a failure empties `vals` AND the holder
  template <class T>
  int upload_values(DevBuf<T>& vals, const T* src, bool src_on_device = false, const char* who = nullptr, const char* what = nullptr) {
    vals.reset();
    int rc = held() ? 0 : fail(-1, "upload_values: no matrix held");
    if (!rc) rc = alloc_array(vals, (size_t)std::max<int64_t>(nnz, 1), who, what);
    if (!rc && nnz && src) rc = copy_in(vals.p, src, (size_t)nnz * sizeof(T), src_on_device);
    if (rc) { vals.reset(); drop(); }
    return rc;
  }
};
