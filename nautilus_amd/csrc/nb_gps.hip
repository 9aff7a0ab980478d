// Gaussian-process likelihood of a long ORDERED series: the kernel around the
// filter of nb_gps_filter.h, which states the recursion and the mapping, and
// the dispatch over its instantiations -- the 4 single kernels and the 23
// multisets of two or three with at most NB_GPS_MAX_STATES states.
#include "../../include/nautilus_hip.h"
#include "nb_common.h"
#include "nb_gps_filter.h"
#include "nb_launch.h"
#include "nb_layout.h"

namespace {

// The terms <K0, K1, K2> in slot order, -1 for a slot that is not there.  The
// plan comes last: in front of n, log_norm and out it moves them to other
// scalar registers, and the allocator then keeps a spilled scalar (a lane
// read) in the unrolled step loop of some instantiations.
template <int K0, int K1, int K2>
__global__ void __launch_bounds__(64)
nb_gps_kernel(const double* __restrict__ tab, int n_data,
              const double* __restrict__ model, long long ld,
              const double* __restrict__ hyper, long long ld_hyper,
              long long n, double log_norm, double* __restrict__ out,
              nb_gps_plan plan) {
  __shared__ double lds[64 * GPS_LS];
  gps_rows<gps_state<K0, K1, K2>>(tab, n_data, model, ld, hyper, ld_hyper,
                                  plan, n, log_norm, out, lds);
}

template <int K0, int K1, int K2>
int launch(const double* tab, int n_data, const nb_gps_plan& plan,
           const double* model, long long ld, const double* hyper,
           long long ld_hyper, long long n, double log_norm, double* out,
           hipStream_t stream) {
  long long b = (n + 63) / 64;
  if (b > (1 << 20)) b = 1 << 20;
  (void)hipGetLastError();
  hipLaunchKernelGGL((nb_gps_kernel<K0, K1, K2>), dim3((unsigned)b), dim3(64),
                     0, stream, tab, n_data, model, ld, hyper, ld_hyper, n,
                     log_norm, out, plan);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

// one digit per slot, 0 for a slot that is not there
constexpr int gps_key(int k0, int k1, int k2) {
  return (k0 + 1) + 5 * (k1 + 1) + 25 * (k2 + 1);
}

}  // namespace

int nb_launch_gps(const double* tab, int n_data, const nb_gps_plan& plan,
                  const double* model, long long ld, const double* hyper,
                  long long ld_hyper, long long n, double log_norm,
                  double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
#define GPS_CASE(K0, K1, K2)                                                 \
  case gps_key(K0, K1, K2):                                                  \
    return launch<K0, K1, K2>(tab, n_data, plan, model, ld, hyper, ld_hyper, \
                              n, log_norm, out, stream);
  switch (gps_key(plan.kind[0], plan.n_terms > 1 ? plan.kind[1] : -1,
                  plan.n_terms > 2 ? plan.kind[2] : -1)) {
    // the 4 single kernels
    GPS_CASE(0, -1, -1) GPS_CASE(1, -1, -1) GPS_CASE(2, -1, -1)
    GPS_CASE(3, -1, -1)
    // the 10 pairs
    GPS_CASE(0, 0, -1) GPS_CASE(0, 1, -1) GPS_CASE(0, 2, -1)
    GPS_CASE(0, 3, -1) GPS_CASE(1, 1, -1) GPS_CASE(1, 2, -1)
    GPS_CASE(1, 3, -1) GPS_CASE(2, 2, -1) GPS_CASE(2, 3, -1)
    GPS_CASE(3, 3, -1)
    // the 13 triples of at most NB_GPS_MAX_STATES states
    GPS_CASE(0, 0, 0) GPS_CASE(0, 0, 1) GPS_CASE(0, 0, 2) GPS_CASE(0, 0, 3)
    GPS_CASE(0, 1, 1) GPS_CASE(0, 1, 2) GPS_CASE(0, 1, 3) GPS_CASE(0, 2, 3)
    GPS_CASE(0, 3, 3) GPS_CASE(1, 1, 1) GPS_CASE(1, 1, 3) GPS_CASE(1, 3, 3)
    GPS_CASE(3, 3, 3)
  }
#undef GPS_CASE
  nb_set_error("no Gaussian-process series likelihood kernel for these terms "
               "(sorted kernel codes, at most %d states)", NB_GPS_MAX_STATES);
  return NB_ERR_ARG;
}
