// C ABI of the hot path (include/nautilus_hip.h): the handles -- bounds, bound
// lists, prior and likelihood tables -- their uploads, and the launches that
// need a handle.  The images are packed by nb_pack.h, and an export that needs
// no handle lives beside its kernel.  No torch types, no exceptions across the
// boundary.
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_pack.h"

#include <cstdarg>
#include <cstdio>
#include <csignal>
#include <ctime>
#include <execinfo.h>
#include <unistd.h>
#include <string>
#include <vector>

static thread_local std::string g_error;

void nb_set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
}

struct nb_bound {
  BoundLayout at;                           // of the blob
  double* blob_dev = nullptr;
  const double** self_list_dev = nullptr;   // device array {blob_dev}
  // two-stage queries: the bound's (neural bound) groups, {0} as group base
  FastGroup* groups_dev = nullptr;
  int* group_base_dev = nullptr;
  int group_base[2] = {0, 0};               // host copy: {0, n_groups}
  int n_groups = 0;
};

struct nb_boundlist {
  const double** ptrs_dev = nullptr;
  int n = 0, dt = 0, n_dim = 0;
  int blocks_single = 0;   // n == 1: ellipsoid blocks (K + M) of the bound
  // two-stage queries: groups of all bounds in list order, first group of
  // every bound (n + 1 entries; host copy for splitting long lists)
  FastGroup* groups_dev = nullptr;
  int* group_base_dev = nullptr;
  std::vector<int> group_base;
  int n_groups = 0;
  const double* blob0 = nullptr;   // any blob of the list (n_dim, strides)
};

// groups of one bound, appended to `out`
static void nb_append_groups(const nb_bound* b, int pos,
                             std::vector<FastGroup>& out) {
  const BoundLayout& at = b->at;
  if (at.E < 1) return;
  for (int m = 0; m < at.M; ++m) {
    FastGroup g;
    g.nb = b->blob_dev + at.off_neural + (int64_t)m * at.neural_stride;
    g.shift = at.periodic ? b->blob_dev + at.off_shift : nullptr;
    g.E = at.E;
    g.b = pos;
    out.push_back(g);
  }
}

// counters of the bound-evaluation kernels (nb_launch.h, nb_set_eval_counters)
static unsigned long long* g_eval_counters = nullptr;
void nb_eval_set_counters(unsigned long long* dev) { g_eval_counters = dev; }
unsigned long long* nb_eval_counters() { return g_eval_counters; }

namespace {

inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }

// What a list query leaves (nautilus_hip.h, nb_list_eval: status 2 = inside,
// first bound INT32_MAX = none) as nb_contains* / nb_first_containing return
// it, in place: masks of 0 / 1, -1 for no bound
__global__ void nb_query_out_kernel(unsigned char* mask, int* idx,
                                    long long n) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  if (mask != nullptr) mask[i] = (mask[i] & 2) != 0 ? 1 : 0;
  if (idx != nullptr && idx[i] == INT32_MAX) idx[i] = -1;
}

// One device allocation of n elements (and `slack` zeroed ones after them)
// filled from the host; freed again if that fails
template <class T>
hipError_t upload_array(T** dev, const T* host, size_t n, size_t slack = 0) {
  hipError_t e = hipMalloc((void**)dev, (n + slack) * sizeof(T));
  if (e == hipSuccess && slack > 0)
    e = hipMemset(*dev + n, 0, slack * sizeof(T));
  if (e == hipSuccess)
    e = hipMemcpy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess && *dev != nullptr) {
    (void)hipFree(*dev);
    *dev = nullptr;
  }
  return e;
}

// The tail of every table create: given what the packer returned, the upload
// of its image and the handle (a copy of `h` with the device pointer set) ...
template <class H, class T>
int nb_make_table(int rc, const std::vector<T>& image, const char* what,
                  H h, H** out) {
  if (out != nullptr) *out = nullptr;
  if (rc != NB_OK) return rc;
  const hipError_t e = upload_array((T**)&h.dev, image.data(), image.size());
  if (e != hipSuccess) {
    nb_set_error("%s upload failed: %s", what, hipGetErrorString(e));
    return NB_ERR_HIP;
  }
  *out = new H(h);
  return NB_OK;
}

// ... which is released with it
template <class H>
int nb_destroy_table(H* h) {
  if (h == nullptr) return NB_OK;
  (void)hipFree(h->dev);
  delete h;
  return NB_OK;
}

}  // namespace

extern "C" {

int nb_abi_version(void) { return NB_ABI_VERSION; }

const char* nb_last_error(void) { return g_error.c_str(); }

int nb_bound_create(const nb_bound_desc* d, nb_bound** out) {
  if (d == nullptr || out == nullptr) {
    nb_set_error("null argument");
    return NB_ERR_ARG;
  }
  BoundLayout at;
  std::vector<double> buf;
  const int rc = pack_bound(d, &at, &buf);
  if (rc != NB_OK) return rc;
  nb_bound* b = new nb_bound();
  b->at = at;
  // (nb_eval_fast.hip stages parts of the blob in whole 1 KB pieces -- the
  // weights, the ellipsoid block -- so the last piece of the last block may
  // read up to 1 KB past its end: keep that inside the allocation)
  constexpr size_t SLACK = 512;
  hipError_t e = upload_array(&b->blob_dev, buf.data(), buf.size(), SLACK);
  if (e == hipSuccess) {
    const double* self = b->blob_dev;
    e = upload_array(&b->self_list_dev, &self, 1);
  }
  if (e == hipSuccess) {
    std::vector<FastGroup> groups;
    nb_append_groups(b, 0, groups);
    b->n_groups = (int)groups.size();
    b->group_base[1] = b->n_groups;
    e = upload_array(&b->group_base_dev, b->group_base, 2);
    if (e == hipSuccess && b->n_groups > 0)
      e = upload_array(&b->groups_dev, groups.data(), groups.size());
  }
  if (e != hipSuccess) {
    nb_set_error("bound upload failed: %s", hipGetErrorString(e));
    nb_bound_destroy(b);
    return NB_ERR_HIP;
  }
  *out = b;
  return NB_OK;
}

int nb_bound_destroy(nb_bound* b) {
  if (b == nullptr) return NB_OK;
  if (b->blob_dev) (void)hipFree(b->blob_dev);
  if (b->self_list_dev) (void)hipFree(b->self_list_dev);
  if (b->groups_dev) (void)hipFree(b->groups_dev);
  if (b->group_base_dev) (void)hipFree(b->group_base_dev);
  delete b;
  return NB_OK;
}

int64_t nb_bound_nbytes(const nb_bound* b) {
  return b ? b->at.total * (int64_t)sizeof(double) : 0;
}

int nb_boundlist_create(nb_bound* const* bounds, int32_t n,
                        nb_boundlist** out) {
  if (n < 0 || (n > 0 && bounds == nullptr) || out == nullptr) {
    nb_set_error("bad bound list");
    return NB_ERR_ARG;
  }
  nb_boundlist* l = new nb_boundlist();
  l->n = n;
  std::vector<const double*> ptrs(n);
  for (int i = 0; i < n; ++i) {
    if (i > 0 && bounds[i]->at.n_dim != bounds[0]->at.n_dim) {
      nb_set_error("bounds of a list must share n_dim");
      delete l;
      return NB_ERR_ARG;
    }
    ptrs[i] = bounds[i]->blob_dev;
  }
  if (n > 0) {
    l->dt = bounds[0]->at.dt;
    l->n_dim = bounds[0]->at.n_dim;
    l->blob0 = bounds[0]->blob_dev;
    if (n == 1) l->blocks_single = bounds[0]->at.K + bounds[0]->at.M;
    std::vector<FastGroup> groups;
    l->group_base.assign(1, 0);
    for (int i = 0; i < n; ++i) {
      nb_append_groups(bounds[i], i, groups);
      l->group_base.push_back((int)groups.size());
    }
    l->n_groups = (int)groups.size();
    hipError_t e = upload_array(&l->ptrs_dev, ptrs.data(), ptrs.size());
    if (e == hipSuccess)
      e = upload_array(&l->group_base_dev, l->group_base.data(),
                       l->group_base.size());
    if (e == hipSuccess && l->n_groups > 0)
      e = upload_array(&l->groups_dev, groups.data(), groups.size());
    if (e != hipSuccess) {
      nb_set_error("bound list upload failed: %s", hipGetErrorString(e));
      nb_boundlist_destroy(l);
      return NB_ERR_HIP;
    }
  }
  *out = l;
  return NB_OK;
}

int nb_boundlist_destroy(nb_boundlist* l) {
  if (l == nullptr) return NB_OK;
  if (l->ptrs_dev) (void)hipFree(l->ptrs_dev);
  if (l->groups_dev) (void)hipFree(l->groups_dev);
  if (l->group_base_dev) (void)hipFree(l->group_base_dev);
  delete l;
  return NB_OK;
}

// debugging aid: native backtrace on SIGABRT / SIGSEGV (NB_ABORT_TRACE=1)
static void nb_abort_trace(int sig) {
  void* frames[64];
  const int n = backtrace(frames, 64);
  const char msg[] = "[nautilus_hip] fatal signal, native backtrace:\n";
  (void)!write(2, msg, sizeof msg - 1);
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}

// (not an export: installed when the library is loaded with NB_ABORT_TRACE set)
__attribute__((constructor)) static void nb_install_abort_trace(void) {
  if (getenv("NB_ABORT_TRACE") == nullptr) return;
  signal(SIGABRT, nb_abort_trace);
  signal(SIGSEGV, nb_abort_trace);
}

// ---- two-stage queries (nb_cand.hip + nb_eval_fast.hip BATCH) --------------
// groups per slice of a long list: the second stage's pass table holds 1024
// (NB_LIST_SLICE_GROUPS lowers it: the test of the slicing itself)
static int nb_slice_groups() {
  const char* e = getenv("NB_LIST_SLICE_GROUPS");
  const int v = e != nullptr ? atoi(e) : 1024;
  return v < 1 ? 1 : (v > 1024 ? 1024 : v);
}
#define NB_SLICE_GROUPS nb_slice_groups()

// What a list query walks: the bounds of a list, or one bound as the list of
// itself
struct ListView {
  const double* const* ptrs_dev;
  int n, dt, n_dim;
  const int* group_base_dev;
  const int* group_base;           // host copy, n + 1 entries
  const FastGroup* groups_dev;
  int n_groups;
  const double* blob0;             // any blob of the list (n_dim, strides)
};

static ListView nb_view_of_list(const nb_boundlist* l) {
  return {l->ptrs_dev, l->n, l->dt, l->n_dim, l->group_base_dev,
          l->group_base.data(), l->groups_dev, l->n_groups, l->blob0};
}

static ListView nb_view_of_bound(const nb_bound* b) {
  return {b->self_list_dev, 1, b->at.dt, b->at.n_dim, b->group_base_dev,
          b->group_base, b->groups_dev, b->n_groups, b->blob_dev};
}

static int64_t nb_view_work_bytes(const ListView& v, int64_t n) {
  const int g = v.n_groups < NB_SLICE_GROUPS ? v.n_groups : NB_SLICE_GROUPS;
  // (a slice never splits a bound: allow for the largest bound's groups)
  int most = 0;
  for (int i = 0; i < v.n; ++i) {
    const int k = v.group_base[i + 1] - v.group_base[i];
    most = k > most ? k : most;
  }
  return nb_cand_work_bytes(v.dt, 0, n, (g > most ? g : most) + 1);
}

int64_t nb_list_eval_work_bytes(const nb_boundlist* l, int64_t n) {
  return nb_view_work_bytes(nb_view_of_list(l), n);
}

int64_t nb_accept_staged_work_bytes(const nb_bound* b, int64_t n) {
  return nb_cand_work_bytes(b->at.dt, 2, n, b->n_groups + 1);
}

static int nb_stage_two(const double* blob0, int n_dim, int recentre,
                        const double* x, const FastGroup* groups, int n_groups,
                        int* totals, int* dense, long long n_pad, long long n,
                        int mode, uint8_t* st, int32_t* first,
                        hipStream_t stream) {
  if (n_groups == 0) return NB_OK;
  // every row is a candidate of every group at most once
  return nb_launch_eval_fast_batch(blob0, n_dim, recentre, x, groups, n_groups,
                                   totals, dense, n_pad,
                                   (long long)n * (n_groups < 8 ? n_groups : 8),
                                   mode, st, first, stream);
}

// NB_STAGE_TIMING=1 (debugging aid): HIP events around the two stages of
// nb_accept_staged; the times of a call are printed two calls later, so that
// nothing waits for the device inside the measured sequence
class StageTimer {
 public:
  explicit StageTimer(hipStream_t stream) : stream_(stream) {
    static const bool timing = getenv("NB_STAGE_TIMING") != nullptr;
    if (!timing) return;
    if (calls_ == 0)
      for (int i = 0; i < 9; ++i) (void)hipEventCreate(&ev_[i / 3][i % 3]);
    if (calls_ > 1) {
      // call k - 2 and the gap to call k - 1 (both finished or in flight
      // behind nothing this call waits for but their own events)
      hipEvent_t* p = ev_[(calls_ - 2) % 3];
      hipEvent_t* q = ev_[(calls_ - 1) % 3];
      const double* h = host_us_[(calls_ - 2) % 3];
      const double* hq = host_us_[(calls_ - 1) % 3];
      float t_geo = 0.f, t_emu = 0.f, t_gap = 0.f;
      (void)hipEventSynchronize(q[0]);
      (void)hipEventElapsedTime(&t_geo, p[0], p[1]);
      (void)hipEventElapsedTime(&t_emu, p[1], p[2]);
      (void)hipEventElapsedTime(&t_gap, p[2], q[0]);
      fprintf(stderr, "[stage] call %d: device: candidates + compaction %.3f "
              "ms, batched scores %.3f ms, then idle until the next call's "
              "first event %.3f ms; host: stage-one launches %.0f us, "
              "stage-two launch %.0f us, until the next call %.0f us\n",
              calls_ - 2, t_geo, t_emu, t_gap, h[1] - h[0], h[2] - h[1],
              hq[0] - h[2]);
    }
    e_ = ev_[calls_ % 3];
    hu_ = host_us_[calls_ % 3];
    ++calls_;
    hu_[0] = now_us();
    (void)hipEventRecord(e_[0], stream_);
  }
  // after stage i (1, 2)
  void mark(int i) {
    if (e_ == nullptr) return;
    (void)hipEventRecord(e_[i], stream_);
    hu_[i] = now_us();
  }

 private:
  static double now_us() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
  }
  static inline hipEvent_t ev_[3][3];
  static inline double host_us_[3][4];
  static inline int calls_ = 0;
  hipStream_t stream_;
  hipEvent_t* e_ = nullptr;
  double* hu_ = nullptr;
};

// The two stages over a non-empty view, in slices of at most NB_SLICE_GROUPS
// groups each: status bytes, and with mode 1 the first containing bound, as
// nb_list_eval documents them.  `work`: nb_view_work_bytes(v, n) bytes.
static int nb_view_eval(const ListView& v, int mode, const double* x,
                        int64_t n, uint8_t* st, int32_t* first, void* work,
                        hipStream_t stream) {
  int b0 = 0;
  while (b0 < v.n) {
    int b1 = b0 + 1;
    while (b1 < v.n && v.group_base[b1 + 1] - v.group_base[b0] <=
                           NB_SLICE_GROUPS)
      ++b1;
    const int g0 = v.group_base[b0], ng = v.group_base[b1] - g0;
    int *dense = nullptr, *totals = nullptr;
    long long n_pad = 0;
    int rc = nb_launch_cand(v.dt, v.n_dim, v.ptrs_dev + b0,
                            v.group_base_dev + b0, b1 - b0, ng, b0, g0,
                            b0 > 0 ? 1 : 0, mode, x, n, st, first, (int*)work,
                            0, 0, &dense, &totals, &n_pad, stream);
    if (rc != NB_OK) return rc;
    rc = nb_stage_two(v.blob0, v.n_dim, 1, x, v.groups_dev + g0, ng, totals,
                      dense, n_pad, n, mode, st, first, stream);
    if (rc != NB_OK) return rc;
    b0 = b1;
  }
  return NB_OK;
}

int nb_list_eval(const nb_boundlist* l, int32_t mode, const double* x,
                 int64_t n, uint8_t* st, int32_t* first, void* work,
                 int64_t work_bytes, void* stream) {
  if (mode != 0 && mode != 1) {
    nb_set_error("nb_list_eval: mode must be 0 (any) or 1 (first)");
    return NB_ERR_ARG;
  }
  if (mode == 1 && first == nullptr) {
    nb_set_error("nb_list_eval: mode 1 needs the `first` output");
    return NB_ERR_ARG;
  }
  if (n <= 0) return NB_OK;
  if (l->n == 0) {
    NB_HIP_CHECK(hipMemsetAsync(st, 0, (size_t)n, as_stream(stream)));
    if (first != nullptr)
      NB_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)first, 0x7fffffff,
                                     (size_t)n, as_stream(stream)));
    return NB_OK;
  }
  if (work_bytes < nb_list_eval_work_bytes(l, n)) {
    nb_set_error("nb_list_eval: work space of %lld bytes, need %lld",
                 (long long)work_bytes,
                 (long long)nb_list_eval_work_bytes(l, n));
    return NB_ERR_ARG;
  }
  return nb_view_eval(nb_view_of_list(l), mode, x, n, st, first, work,
                      as_stream(stream));
}

int nb_accept_staged(const nb_bound* b, uint64_t seed, uint64_t offset,
                     const double* x, int64_t n, uint8_t* flags, void* work,
                     int64_t work_bytes, int64_t* totals_offset, void* stream) {
  if (n <= 0) return NB_OK;
  if (work_bytes < nb_accept_staged_work_bytes(b, n)) {
    nb_set_error("nb_accept_staged: work space of %lld bytes, need %lld",
                 (long long)work_bytes,
                 (long long)nb_accept_staged_work_bytes(b, n));
    return NB_ERR_ARG;
  }
  int *dense = nullptr, *totals = nullptr;
  long long n_pad = 0;
  StageTimer timer(as_stream(stream));
  int rc = nb_launch_cand(b->at.dt, b->at.n_dim, b->self_list_dev,
                          b->group_base_dev, 1, b->n_groups, 0, 0, 0, 2, x, n,
                          flags, nullptr,
                          (int*)work, seed, offset, &dense, &totals, &n_pad,
                          as_stream(stream));
  if (rc != NB_OK) return rc;
  timer.mark(1);
  if (totals_offset != nullptr)
    *totals_offset = (int64_t)((char*)totals - (char*)work);
  rc = nb_stage_two(b->blob_dev, b->at.n_dim, 0, x, b->groups_dev, b->n_groups,
                    totals, dense, n_pad, n, 2, flags, nullptr,
                    as_stream(stream));
  timer.mark(2);
  return rc;
}

// ---- queries without a work argument ---------------------------------------
// nb_contains, nb_contains_any, nb_first_containing and nb_accept run the same
// two stages in work space allocated and freed in stream order on the
// caller's stream (nothing owned by a handle: streams may share one).
static int nb_scratch_alloc(void** out, int64_t bytes, const char* instead,
                            hipStream_t stream) {
  const hipError_t e = hipMallocAsync(out, (size_t)bytes, stream);
  if (e == hipSuccess) return NB_OK;
  (void)hipGetLastError();
  nb_set_error("%lld bytes of stream-ordered work space: %s (%s takes "
               "caller-owned work space)", (long long)bytes,
               hipGetErrorString(e), instead);
  return NB_ERR_HIP;
}

static int nb_scratch_free(void* work, int rc, hipStream_t stream) {
  const hipError_t e = hipFreeAsync(work, stream);
  if (rc == NB_OK && e != hipSuccess) {
    nb_set_error("hipFreeAsync failed: %s", hipGetErrorString(e));
    return NB_ERR_HIP;
  }
  return rc;
}

// mask != NULL: mask[i] = 1 if any bound of the view contains row i, else 0;
// idx != NULL: idx[i] = first bound that contains row i, -1 if none
static int nb_view_query(const ListView& v, const double* x, int64_t n,
                         uint8_t* mask, int32_t* idx, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  if (v.n == 0) {
    if (mask != nullptr) NB_HIP_CHECK(hipMemsetAsync(mask, 0, (size_t)n, stream));
    if (idx != nullptr)
      NB_HIP_CHECK(hipMemsetAsync(idx, 0xFF, (size_t)n * 4, stream));
    return NB_OK;
  }
  // (a query for the first bound alone: its status bytes live behind the
  // work space, in whole 32-bit words -- the first stage may OR into the word
  // that holds a byte)
  const int64_t work_bytes = nb_view_work_bytes(v, n);
  const int64_t st_bytes = mask == nullptr ? (n + 3) / 4 * 4 : 0;
  void* work = nullptr;
  int rc = nb_scratch_alloc(&work, work_bytes + st_bytes, "nb_list_eval",
                            stream);
  if (rc != NB_OK) return rc;
  uint8_t* st = mask != nullptr ? mask : (uint8_t*)work + work_bytes;
  rc = nb_view_eval(v, idx != nullptr ? 1 : 0, x, n, st, idx, work, stream);
  if (rc == NB_OK) {
    hipLaunchKernelGGL(nb_query_out_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, stream, mask, idx, (long long)n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      nb_set_error("nb_query_out_kernel: %s", hipGetErrorString(e));
      rc = NB_ERR_HIP;
    }
  }
  return nb_scratch_free(work, rc, stream);
}

int nb_contains(const nb_bound* b, const double* x, int64_t n, uint8_t* mask,
                void* stream) {
  return nb_view_query(nb_view_of_bound(b), x, n, mask, nullptr,
                       as_stream(stream));
}

int nb_contains_any(const nb_boundlist* l, const double* x, int64_t n,
                    uint8_t* mask, void* stream) {
  return nb_view_query(nb_view_of_list(l), x, n, mask, nullptr,
                       as_stream(stream));
}

int nb_first_containing(const nb_boundlist* l, const double* x, int64_t n,
                        int32_t* idx, void* stream) {
  return nb_view_query(nb_view_of_list(l), x, n, nullptr, idx,
                       as_stream(stream));
}

int nb_accept(const nb_bound* b, uint64_t seed, uint64_t offset,
              const double* x, int64_t n, uint8_t* flags, void* stream) {
  // one neural bound, at most one outer member: the pipelined kernel
  if (nb_eval_fast_eligible(b->at.n_dim, b->at.K, b->at.M, b->at.E, true))
    return nb_launch_eval_fast(b->blob_dev, b->at.n_dim, true, 0, 0, x,
                               nullptr, n, flags, nullptr, seed, offset,
                               as_stream(stream));
  if (n <= 0) return NB_OK;
  const int64_t work_bytes = nb_accept_staged_work_bytes(b, n);
  void* work = nullptr;
  int rc = nb_scratch_alloc(&work, work_bytes, "nb_accept_staged",
                            as_stream(stream));
  if (rc != NB_OK) return rc;
  rc = nb_accept_staged(b, seed, offset, x, n, flags, work, work_bytes,
                        nullptr, stream);
  return nb_scratch_free(work, rc, as_stream(stream));
}

int nb_member_count(const nb_bound* b, const double* x, int64_t n,
                    uint8_t* count, void* stream) {
  return nb_launch_geom(b->blob_dev, b->at.dt, 1, x, n, nullptr, count,
                        as_stream(stream));
}

int nb_neural_score(const nb_bound* b, const double* x, int64_t n, double* out,
                    void* stream) {
  if (b->at.M < 1) {
    nb_set_error("bound has no neural bound");
    return NB_ERR_ARG;
  }
  // with emulators the pipelined kernel, without them the quadratic form alone
  if (nb_eval_fast_eligible(b->at.n_dim, b->at.K, b->at.M, b->at.E, false))
    return nb_launch_eval_fast(b->blob_dev, b->at.n_dim, false, 0, 0, x,
                               nullptr, n, nullptr, out, 0, 0,
                               as_stream(stream));
  return nb_launch_geom(b->blob_dev, b->at.dt, 0, x, n, out, nullptr,
                        as_stream(stream));
}

int nb_neural_score_rows(const nb_bound* b, int32_t m, int32_t recentre,
                         const double* x, const int64_t* idx, int64_t n,
                         double* out, void* stream) {
  if (m < 0 || m >= b->at.M || b->at.E < 1) {
    nb_set_error("nb_neural_score_rows: neural bound %d of %d (E = %d)", m,
                 b->at.M, b->at.E);
    return NB_ERR_ARG;
  }
  return nb_launch_eval_fast(b->blob_dev, b->at.n_dim, false, m, recentre, x,
                             (const long long*)idx, n, nullptr, out, 0, 0,
                             as_stream(stream));
}

int nb_propose(const nb_bound* b, uint64_t seed, uint64_t offset, int64_t n,
               double* x, void* stream) {
  if (b->at.K < 1) {
    nb_set_error("bound has no outer members to draw from");
    return NB_ERR_ARG;
  }
  return nb_launch_draw(b->blob_dev, b->at.n_dim, seed, offset, n, x,
                        as_stream(stream));
}

int nb_set_eval_counters(uint64_t* counters_dev) {
  nb_eval_set_counters((unsigned long long*)counters_dev);
  return NB_OK;
}

int nb_ellipsoid_transform(const nb_bound* b, const double* x, int64_t n,
                           double* y, void* stream) {
  const double* blk = nullptr;
  if (b->at.single_full)
    blk = b->blob_dev + b->at.off_members;
  else if (b->at.K == 0 && b->at.M >= 1)
    blk = b->blob_dev + b->at.off_neural;
  if (blk == nullptr) {
    nb_set_error("nb_ellipsoid_transform needs an Ellipsoid or a NeuralBound");
    return NB_ERR_ARG;
  }
  return nb_launch_transform(blk, b->at.dt, b->at.n_dim, x, n, y,
                             as_stream(stream));
}

// Device-resident table of a prior (nb_transform.hip, PT_* rows): one
// allocation holding par[NB_PRIOR_NPAR][n_dim], key_value[n_keys],
// key_column[n_keys] and kind[n_dim], in that order (nb_layout.h).
struct nb_prior_table {
  double* dev = nullptr;
  int n_dim = 0, n_keys = 0;
  int level = 0;            // kernel variant: 0 kinds 0 and 2 only, 1 with the
                            // normal families, 2 with log-space truncnorm;
                            // 3 more with a closed-form kind (7 to 17)
  const double* par() const { return dev; }
  const double* key_value() const { return dev + NB_PRIOR_NPAR * (size_t)n_dim; }
  const int* key_column() const { return (const int*)(key_value() + n_keys); }
  const unsigned char* kind() const {
    return (const unsigned char*)(key_column() + n_keys);
  }
};

int nb_prior_table_create(int32_t n_dim, const uint8_t* kind,
                          const double* loc, const double* scale,
                          const double* shape0, const double* shape1,
                          int32_t n_keys, const int32_t* key_column,
                          const double* key_value, nb_prior_table** out) {
  std::vector<unsigned char> image;
  nb_prior_table h;
  const int rc = pack_prior_table(n_dim, kind, loc, scale, shape0, shape1,
                                  n_keys, key_column, key_value, out, &image,
                                  &h.level);
  h.n_dim = n_dim;
  h.n_keys = n_keys;
  return nb_make_table(rc, image, "prior table", h, out);
}

int nb_prior_table_destroy(nb_prior_table* table) {
  return nb_destroy_table(table);
}

int nb_prior_table_transform(const nb_prior_table* table, const double* u,
                             int64_t n, int32_t layout, double* out,
                             void* stream) {
  if (table == nullptr || (layout != NB_PRIOR_ROW_MAJOR &&
                           layout != NB_PRIOR_COLUMN_MAJOR) ||
      n < 0 || (n > 0 && (u == nullptr || out == nullptr))) {
    nb_set_error("bad prior transform arguments");
    return NB_ERR_ARG;
  }
  return nb_launch_prior_table(u, n, table->n_dim, table->par(), table->kind(),
                               table->n_keys, table->key_column(),
                               table->key_value(),
                               layout == NB_PRIOR_COLUMN_MAJOR, table->level,
                               out,
                               as_stream(stream));
}

// Components of a mixture packed for nb_mixture.hip: K records of
// nb_mixture_record(dt) doubles, uploaded once.
struct nb_mixture {
  double* dev = nullptr;
  int n_dim = 0, n_comp = 0;
};

int nb_mixture_create(int32_t n_dim, int32_t n_components, const double* means,
                      const double* chol_inv, const double* log_coef,
                      nb_mixture** out) {
  std::vector<double> image;
  const int rc = pack_mixture(n_dim, n_components, means, chol_inv, log_coef,
                              out, &image);
  nb_mixture h;
  h.n_dim = n_dim;
  h.n_comp = n_components;
  return nb_make_table(rc, image, "mixture", h, out);
}

int nb_mixture_destroy(nb_mixture* mix) { return nb_destroy_table(mix); }

int nb_mixture_loglike(const nb_mixture* mix, const double* x, int64_t n,
                       double* out, int32_t* label, void* stream) {
  if (mix == nullptr || n < 0 || (n > 0 && (x == nullptr || out == nullptr))) {
    nb_set_error("bad mixture likelihood arguments");
    return NB_ERR_ARG;
  }
  return nb_launch_mixture(mix->dev, mix->n_dim, mix->n_comp, x, n, out, label,
                           as_stream(stream));
}

// Data vector and W = L^-1 (or 1 / sigma) packed for nb_chi2.hip
// (nb_layout.h, nb_chi2_w_offset), uploaded once.
struct nb_chi2 {
  double* dev = nullptr;
  int n_data = 0;
  bool diag = false;
  double log_norm = 0.0;
};

int nb_chi2_create(int32_t n_data, const double* data, const double* chol_inv,
                   const double* inv_sigma, double log_norm, nb_chi2** out) {
  std::vector<double> image;
  const int rc = pack_chi2(n_data, data, chol_inv, inv_sigma, log_norm, out,
                           &image);
  nb_chi2 h;
  h.n_data = n_data;
  h.diag = inv_sigma != nullptr;
  h.log_norm = log_norm;
  return nb_make_table(rc, image, "data likelihood", h, out);
}

int nb_chi2_destroy(nb_chi2* h) { return nb_destroy_table(h); }

int nb_chi2_loglike(const nb_chi2* h, const double* model, int64_t ld,
                    int64_t n, double* out, void* stream) {
  if (h == nullptr || n < 0 || ld < h->n_data ||
      (n > 0 && (model == nullptr || out == nullptr))) {
    nb_set_error("bad data likelihood arguments (ld >= n_data)");
    return NB_ERR_ARG;
  }
  if (h->diag)
    return nb_launch_chi2_diag(h->dev, h->n_data, model, ld, n, h->log_norm,
                               out, as_stream(stream));
  return nb_launch_chi2(h->dev, h->n_data, model, ld, n, h->log_norm, out,
                        as_stream(stream));
}

// Counts, their reciprocals, exposure and background for nb_poisson.hip,
// uploaded once.
struct nb_poisson {
  double* dev = nullptr;
  int n_data = 0;
  double log_const = 0.0;
};

int nb_poisson_create(int32_t n_data, const double* counts,
                      const double* exposure, const double* background,
                      double log_const, nb_poisson** out) {
  std::vector<double> image;
  const int rc = pack_poisson(n_data, counts, exposure, background, log_const,
                              out, &image);
  nb_poisson h;
  h.n_data = n_data;
  h.log_const = log_const;
  return nb_make_table(rc, image, "Poisson likelihood", h, out);
}

int nb_poisson_destroy(nb_poisson* h) { return nb_destroy_table(h); }

int nb_poisson_loglike(const nb_poisson* h, const double* model, int64_t ld,
                       int64_t n, double* out, void* stream) {
  if (h == nullptr || n < 0 || (n > 1 && ld < h->n_data) ||
      (n > 0 && (model == nullptr || out == nullptr))) {
    nb_set_error("bad Poisson likelihood arguments (ld >= n_data)");
    return NB_ERR_ARG;
  }
  return nb_launch_poisson(h->dev, h->n_data, model, ld, n, h->log_const, out,
                           as_stream(stream));
}

// The table of nb_poisson and the response matrix packed for nb_fold.hip
// (nb_layout.h, nb_fold_r_offset), uploaded once.
struct nb_fold_poisson {
  double* dev = nullptr;
  int n_data = 0;
  int n_src = 0;
  double log_const = 0.0;
};

int nb_fold_poisson_create(int32_t n_data, int32_t n_src, const double* counts,
                           const double* response, int64_t ld_response,
                           const double* exposure, const double* background,
                           double log_const, nb_fold_poisson** out) {
  std::vector<double> image;
  const int rc = pack_fold_poisson(n_data, n_src, counts, response, ld_response,
                                   exposure, background, log_const, out,
                                   &image);
  nb_fold_poisson h;
  h.n_data = n_data;
  h.n_src = n_src;
  h.log_const = log_const;
  return nb_make_table(rc, image, "folded Poisson likelihood", h, out);
}

int nb_fold_poisson_destroy(nb_fold_poisson* h) { return nb_destroy_table(h); }

int nb_fold_poisson_loglike(const nb_fold_poisson* h, const double* src,
                            int64_t ld, int64_t n, double* out, void* stream) {
  if (h == nullptr || n < 0 || (n > 1 && ld < h->n_src) ||
      (n > 0 && (src == nullptr || out == nullptr))) {
    nb_set_error("bad folded Poisson likelihood arguments (ld >= n_src)");
    return NB_ERR_ARG;
  }
  return nb_launch_fold_poisson(h->dev, h->n_data, h->n_src, src, ld, n,
                                h->log_const, out, as_stream(stream));
}

// Data and sigma^2 for nb_noise.hip, uploaded once.
struct nb_noise {
  double* dev = nullptr;
  int n_data = 0;
  double log_norm = 0.0;
};

int nb_noise_create(int32_t n_data, const double* data, const double* sigma2,
                    double log_norm, nb_noise** out) {
  std::vector<double> image;
  const int rc = pack_noise(n_data, data, sigma2, log_norm, out, &image);
  nb_noise h;
  h.n_data = n_data;
  h.log_norm = log_norm;
  return nb_make_table(rc, image, "noise likelihood", h, out);
}

int nb_noise_destroy(nb_noise* h) { return nb_destroy_table(h); }

int nb_noise_loglike(const nb_noise* h, int32_t mode, const double* model,
                     int64_t ld, const double* noise, int64_t ld_noise,
                     int64_t n, double* out, void* stream) {
  if (h == nullptr || n < 0 ||
      (mode != NB_NOISE_ROW && mode != NB_NOISE_FULL)) {
    nb_set_error("bad noise likelihood arguments (a handle, n >= 0, mode "
                 "NB_NOISE_ROW or NB_NOISE_FULL)");
    return NB_ERR_ARG;
  }
  const int64_t width = mode == NB_NOISE_ROW ? 3 : h->n_data;
  if ((n > 1 && (ld < h->n_data || ld_noise < width)) ||
      (n > 0 && (model == nullptr || noise == nullptr || out == nullptr))) {
    nb_set_error("bad noise likelihood arguments (ld >= n_data, ld_noise >= "
                 "%lld, no NULL pointer)", (long long)width);
    return NB_ERR_ARG;
  }
  return nb_launch_noise(h->dev, h->n_data, mode, model, ld, noise, ld_noise,
                         n, h->log_norm, out, as_stream(stream));
}

// nb_outlier.hip reads the table of nb_noise.hip
int nb_outlier_loglike(const nb_noise* h, const double* model, int64_t ld,
                       const double* mix, int64_t ld_mix, int64_t n,
                       double* out, void* stream) {
  if (h == nullptr || n < 0 ||
      (n > 1 && (ld < h->n_data || ld_mix < NB_OUTLIER_WIDTH)) ||
      (n > 0 && (model == nullptr || mix == nullptr || out == nullptr))) {
    nb_set_error("bad outlier likelihood arguments (a handle, n >= 0, ld >= "
                 "n_data, ld_mix >= %d, no NULL pointer)", NB_OUTLIER_WIDTH);
    return NB_ERR_ARG;
  }
  return nb_launch_outlier(h->dev, h->n_data, model, ld, mix, ld_mix, n,
                           h->log_norm, out, as_stream(stream));
}

// Data, sigma^2 and the distance tiles for nb_gp.hip (nb_layout.h,
// nb_gp_tile), uploaded once.
struct nb_gp {
  double* dev = nullptr;
  int n_data = 0;
  int kernel = 0;
  bool has_dist = false;
  double log_norm = 0.0;
};

int nb_gp_create(int32_t n_data, const double* data, const double* sigma2,
                 const double* dist, int32_t kernel, double log_norm,
                 nb_gp** out) {
  std::vector<double> image;
  const int rc = pack_gp(n_data, data, sigma2, dist, kernel, log_norm, out,
                         &image);
  nb_gp h;
  h.n_data = n_data;
  h.kernel = kernel;
  h.has_dist = dist != nullptr;
  h.log_norm = log_norm;
  return nb_make_table(rc, image, "Gaussian-process likelihood", h, out);
}

int nb_gp_destroy(nb_gp* h) { return nb_destroy_table(h); }

int nb_gp_loglike(const nb_gp* h, int32_t mode, const double* model,
                  int64_t ld, const double* cov, int64_t ld_cov, int64_t n,
                  double* out, void* stream) {
  if (h == nullptr || n < 0 || (mode != NB_GP_HYPER && mode != NB_GP_FULL)) {
    nb_set_error("bad Gaussian-process likelihood arguments (a handle, "
                 "n >= 0, mode NB_GP_HYPER or NB_GP_FULL)");
    return NB_ERR_ARG;
  }
  if (mode == NB_GP_HYPER && !h->has_dist) {
    nb_set_error("bad Gaussian-process likelihood arguments (NB_GP_HYPER "
                 "needs a handle created with dist)");
    return NB_ERR_ARG;
  }
  const int64_t width =
      mode == NB_GP_HYPER ? 3 : (int64_t)h->n_data * h->n_data;
  if ((n > 1 && (ld < h->n_data || ld_cov < width)) ||
      (n > 0 && (model == nullptr || cov == nullptr || out == nullptr))) {
    nb_set_error("bad Gaussian-process likelihood arguments (ld >= n_data, "
                 "ld_cov >= %lld, no NULL pointer)", (long long)width);
    return NB_ERR_ARG;
  }
  return nb_launch_gp(h->dev, h->n_data, h->kernel, mode, model, ld, cov,
                      ld_cov, n, h->log_norm, out, as_stream(stream));
}

// Steps, data and sigma^2 for nb_gps_filter.h (nb_layout.h, NB_GPS_STRIDE),
// uploaded once, and where a hyper row holds the terms.
struct nb_gps {
  double* dev = nullptr;
  int n_data = 0;
  double log_norm = 0.0;
  nb_gps_plan plan;
};

int nb_gps_create(int32_t n_data, const double* t, const double* data,
                  const double* sigma2, int32_t kernel, double log_norm,
                  nb_gps** out) {
  std::vector<double> image;
  const int rc = pack_gps(n_data, t, data, sigma2, kernel, log_norm, out,
                          &image);
  nb_gps h;
  h.n_data = n_data;
  h.log_norm = log_norm;
  h.plan = plan_gps_one(kernel);
  return nb_make_table(rc, image, "Gaussian-process series likelihood", h,
                       out);
}

int nb_gps_create_terms(int32_t n_data, const double* t, const double* data,
                        const double* sigma2, int32_t n_terms,
                        const int32_t* kernels, double log_norm,
                        nb_gps** out) {
  nb_gps h;
  int rc = plan_gps_terms(n_terms, kernels, t, data, out, &h.plan);
  if (rc != NB_OK) return rc;
  std::vector<double> image;
  rc = pack_gps(n_data, t, data, sigma2, h.plan.kind[0], log_norm, out,
                &image);
  h.n_data = n_data;
  h.log_norm = log_norm;
  return nb_make_table(rc, image, "Gaussian-process series likelihood", h,
                       out);
}

int nb_gps_destroy(nb_gps* h) { return nb_destroy_table(h); }

int nb_gps_loglike(const nb_gps* h, const double* model, int64_t ld,
                   const double* hyper, int64_t ld_hyper, int64_t n,
                   double* out, void* stream) {
  if (h == nullptr || n < 0) {
    nb_set_error("bad Gaussian-process series likelihood arguments (a "
                 "handle, n >= 0)");
    return NB_ERR_ARG;
  }
  const int64_t width = h->plan.width;
  if ((n > 1 && (ld < h->n_data || ld_hyper < width)) ||
      (n > 0 && (model == nullptr || hyper == nullptr || out == nullptr))) {
    nb_set_error("bad Gaussian-process series likelihood arguments (ld >= "
                 "n_data, ld_hyper >= %lld, no NULL pointer)",
                 (long long)width);
    return NB_ERR_ARG;
  }
  return nb_launch_gps(h->dev, h->n_data, h->plan, model, ld, hyper,
                       ld_hyper, n, h->log_norm, out, as_stream(stream));
}

int nb_ellipsoid_contains_stream(const nb_bound* b, const double* x, int64_t n,
                                 uint8_t* mask, void* stream) {
  if (!b->at.single_full) {
    nb_set_error("nb_ellipsoid_contains_stream needs a single full ellipsoid");
    return NB_ERR_ARG;
  }
  const double* cvec = b->blob_dev + b->at.off_stream;
  return nb_launch_ell_stream(cvec, cvec + 16 * b->at.dt, b->at.n_dim, x, n,
                              mask, as_stream(stream));
}

}  // extern "C"
