// devmem_check.cpp -- the owning device buffer and the CSR holder of the library (ganmf_amd/csrc/lib/devmem.inc), checked on the host:
// the file is included over a shim that defines the handful of HIP names it uses on the host heap.  The shim keeps the set of live
// pointers, aborts on a free of a pointer it does not hold, and can be told to fail the k-th allocation or the k-th copy.  Built by
// tests/test_devmem_host.py with -fsanitize=address,undefined.  Every case prints "ok   <name>" and the program ends with
// "all cases clean"; a broken property prints "FAIL ..." and the exit status is 1.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// ---- the shim ------------------------------------------------------------------------------------------------------------------------
typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToDevice = 3 };
enum { hipHostMallocDefault = 0 };

static std::map<void*, size_t> g_live;      // pointer -> bytes, device and pinned alike
static long long g_allocs = 0;              // allocations asked for so far
static long long g_fail_alloc = -1;         // the allocation with this index fails (-1: none)
static long long g_copies = 0;              // copies asked for so far
static long long g_fail_copy = -1;          // the copy with this index fails (-1: none)
static int g_syncs = 0;

static hipError_t shim_alloc(void** p, size_t bytes) {
  if (g_allocs++ == g_fail_alloc) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes);
  std::memset(*p, 0xA5, bytes);             // never zero by accident
  g_live[*p] = bytes;
  return hipSuccess;
}
static hipError_t shim_free(void* p) {
  if (!p) return hipSuccess;
  if (!g_live.count(p)) { std::printf("FAIL free of a pointer that is not held\n"); std::abort(); }
  g_live.erase(p);
  std::free(p);
  return hipSuccess;
}
static hipError_t hipMalloc(void** p, size_t bytes) { return shim_alloc(p, bytes); }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return shim_alloc(p, bytes); }
static hipError_t hipFree(void* p) { return shim_free(p); }
static hipError_t hipHostFree(void* p) { return shim_free(p); }
static hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  if (g_copies++ == g_fail_copy) return hipErrorInvalidValue;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
static hipError_t hipMemset(void* dst, int v, size_t bytes) { std::memset(dst, v, bytes); return hipSuccess; }
static hipError_t hipDeviceSynchronize() { ++g_syncs; return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t) { ++g_syncs; return hipSuccess; }
static hipError_t hipGetLastError() { return hipSuccess; }
static const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e ? "invalid value" : "no error"; }

static std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(-2, "%s failed: %s", #x, hipGetErrorString(e_)); } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_ != 0) return rc_; } while (0)

#include "../ganmf_amd/csrc/lib/devmem.inc"

// ---- the cases -----------------------------------------------------------------------------------------------------------------------
static int g_failed = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                       \
      std::printf("\n");                              \
      g_failed = 1;                                   \
    }                                                 \
  } while (0)

static long long live() { return g_live_device_bytes.load(); }
static void nothing_live(const char* name) {
  CHECK(live() == 0, "%s: %lld bytes counted live", name, live());
  CHECK(g_live.empty(), "%s: %zu pointers still held", name, g_live.size());
  if (!g_failed) std::printf("ok   %s\n", name);
}

static void case_lifetimes() {
  {
    DevBuf<float> a;
    CHECK(a.alloc(100, true) == 0 && a.p && a.cap == 100, "alloc");
    CHECK(live() == 400, "100 floats count %lld bytes", live());
    float* const first = a;                 // reads as a plain pointer
    CHECK(first == a.get(), "conversion");
    CHECK(a.grow(nullptr, 50, true) == 0 && a.get() == first && a.cap == 100, "a grow that fits changes nothing");
    const int syncs = g_syncs;
    CHECK(a.grow(nullptr, 200, false) == 0 && a.cap == 200 && live() == 800, "a grow that does not fit replaces the array");
    CHECK(g_syncs == syncs + 1, "the stream is drained before the old array is freed");
    DevBuf<float> b;
    CHECK(b.alloc(1, false) == 0 && live() == 800 + 16, "an allocation holds at least 16 bytes: %lld", live());
    b = std::move(a);                       // into a non-empty buffer: its array is freed
    CHECK(!a.p && a.cap == 0 && b.cap == 200 && live() == 800, "move-assignment");
    DevBuf<float> c(std::move(b));
    CHECK(!b.p && c.cap == 200 && live() == 800, "move-construction");
    c.reset();
    CHECK(!c.p && c.cap == 0 && live() == 0, "reset");
    c.reset();                              // twice: nothing to free
    DevBuf<double> d;
    CHECK(d.alloc("who", "what", 3) == 0 && d.cap == 3 && live() == 24, "the named allocation");
    PinnedBuf<int> s;
    CHECK(s.alloc(64, false) == 0 && s.p && live() == 24, "pinned staging is owned and not counted");
    std::swap(c, b);
  }                                         // the destructors free the rest
  nothing_live("alloc, grow, reset, move: nothing live at the end");
}

static void case_failed_grow() {
  DevBuf<int> a;
  CHECK(a.alloc(10, false) == 0, "alloc");
  g_fail_alloc = g_allocs;
  CHECK(a.grow(nullptr, 20, true) != 0, "the grow fails");
  CHECK(!a.p && a.cap == 0 && live() == 0, "a failed grow leaves null and capacity 0");
  CHECK(g_err.find("out of memory") != std::string::npos, "the message names the cause: %s", g_err.c_str());
  g_fail_alloc = g_allocs;
  DevBuf<double> s;
  CHECK(s.alloc("fit", "S", 7) != 0 && !s.p && s.cap == 0, "the named allocation fails");
  CHECK(g_err == "fit: out of memory: S needs 56 bytes (out of memory)", "its message: %s", g_err.c_str());
  g_fail_alloc = -1;
  CHECK(a.grow(nullptr, 20, true) == 0 && a.cap == 20, "and the next one succeeds");
  a.reset();
  nothing_live("a failed grow leaves null with capacity 0");
}

static void case_zeroed() {
  DevBuf<double> a;
  CHECK(a.alloc(33, true) == 0, "alloc");
  bool zero = true;
  for (size_t i = 0; i < 33; ++i) zero = zero && a.p[i] == 0.0;
  CHECK(zero, "zeroed = true zeroes");
  DevBuf<unsigned char> b;
  CHECK(b.alloc(3, true) == 0, "alloc");
  for (size_t i = 0; i < 16; ++i) zero = zero && b.p[i] == 0;      // the whole 16 bytes it holds
  CHECK(zero, "the minimum allocation is zeroed whole");
  DevBuf<unsigned char> c;
  CHECK(c.alloc(16, false) == 0 && c.p[0] == 0xA5, "zeroed = false leaves the bytes alone");
  a.reset(); b.reset(); c.reset();
  nothing_live("the zeroed flag zeroes");
}

struct Host { std::vector<int64_t> ip; std::vector<int32_t> ix; std::vector<float> v; long long rows, cols; };
static Host host_matrix(long long rows, long long cols, int per_row) {
  Host m;
  m.rows = rows; m.cols = cols;
  m.ip.assign((size_t)rows + 1, 0);
  for (long long r = 0; r < rows; ++r) {
    for (int j = 0; j < per_row && j < cols; ++j) { m.ix.push_back(j); m.v.push_back((float)(r + j)); }
    m.ip[(size_t)r + 1] = (int64_t)m.ix.size();
  }
  return m;
}
// as the library's setters do it: the values go with the matrix they belong to
static int hold(DevCsr& c, DevBuf<float>& v, const Host& m) {
  v.reset();
  TRY(c.upload(m.ip.data(), m.ix.data(), m.rows, m.cols));
  return c.upload_values(v, m.v.data());
}
static bool empty(const DevCsr& c, const DevBuf<float>& v) {
  return !c.held() && !c.indptr.p && !c.indices.p && !v.p && c.rows == 0 && c.cols == 0 && c.nnz == 0;
}

static void case_upload() {
  DevCsr c;
  DevBuf<float> v;
  const Host a = host_matrix(5, 7, 3), b = host_matrix(9, 4, 2);
  CHECK(hold(c, v, a) == 0 && c.held() && c.rows == 5 && c.cols == 7 && c.nnz == 15, "upload");
  CHECK(live() == 6 * 8 + 15 * 4 + 15 * 4, "three arrays: %lld", live());
  CHECK(std::memcmp(c.indptr.p, a.ip.data(), 6 * 8) == 0 && std::memcmp(c.indices.p, a.ix.data(), 60) == 0 && std::memcmp(v.p, a.v.data(), 60) == 0, "contents");
  CHECK(hold(c, v, b) == 0 && c.rows == 9 && c.cols == 4 && c.nnz == 18 && live() == 10 * 8 + 18 * 4 + 18 * 4, "a second upload replaces the first");
  // a failure at every allocation of an upload onto a holder that holds a matrix: three allocations
  for (int k = 0; k < 3; ++k) {
    CHECK(hold(c, v, a) == 0, "hold");
    g_fail_alloc = g_allocs + k;
    CHECK(hold(c, v, b) != 0, "allocation %d fails", k);
    g_fail_alloc = -1;
    CHECK(empty(c, v) && live() == 0 && g_live.empty(), "allocation %d failed: the holder is empty and nothing is live (%lld)", k, live());
  }
  // a copy that fails: the row pointers', the indices', the values'
  for (int k = 0; k < 3; ++k) {
    CHECK(hold(c, v, a) == 0, "hold");
    g_fail_copy = g_copies + k;
    CHECK(hold(c, v, b) != 0, "copy %d fails", k);
    g_fail_copy = -1;
    CHECK(empty(c, v) && live() == 0 && g_live.empty(), "copy %d failed: the holder is empty and nothing is live (%lld)", k, live());
  }
  {      // a null index source: the array is allocated for a kernel to fill, nothing is copied into it
    const long long copies = g_copies;
    CHECK(c.upload(b.ip.data(), nullptr, b.rows, b.cols) == 0 && c.nnz == 18 && c.indices.cap == 18 && g_copies == copies + 1, "a null index source");
    c.drop();
  }
  CHECK(c.upload_values(v, a.v.data()) != 0 && empty(c, v), "values without a matrix are refused");
  nothing_live("DevCsr::upload: a failure anywhere leaves an empty holder");
}

static void case_shapes() {
  DevCsr c;
  DevBuf<float> v;
  const Host none = host_matrix(4, 6, 0);      // nnz == 0
  CHECK(hold(c, v, none) == 0 && c.held() && c.rows == 4 && c.cols == 6 && c.nnz == 0, "nnz == 0 uploads");
  CHECK(c.indices.p && v.p && c.indices.cap == 1 && v.cap == 1, "one element where the matrix is empty");
  const Host norows = host_matrix(0, 6, 0);    // rows == 0: indptr = {0}
  CHECK(hold(c, v, norows) == 0 && c.held() && c.rows == 0 && c.cols == 6 && c.nnz == 0 && c.indptr.cap == 1, "rows == 0 uploads");
  const Host last_empty = [] { Host m = host_matrix(3, 5, 2); m.ip[3] = m.ip[2]; m.ix.resize(4); m.v.resize(4); return m; }();
  CHECK(hold(c, v, last_empty) == 0 && c.nnz == 4 && c.indptr.p[3] == 4, "an empty last row");
  std::vector<long long> ll(last_empty.ip.begin(), last_empty.ip.end());
  CHECK(c.upload(ll.data(), last_empty.ix.data(), 3, 5) == 0 && c.nnz == 4, "long long row pointers");
  c.drop(); v.reset();
  CHECK(empty(c, v), "drop");
  nothing_live("the nnz == 0 and rows == 0 shapes");
}

int main() {
  case_lifetimes();
  case_failed_grow();
  case_zeroed();
  case_upload();
  case_shapes();
  if (g_failed) return 1;
  std::printf("all cases clean\n");
  return 0;
}
