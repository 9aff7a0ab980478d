// Launchers and size functions that cross a file boundary: defined beside
// their kernels, called from nb_api.hip (or another kernel file).  The caller
// and the defining file both include this header, so a signature that drifts
// is a compile error.
#pragma once

#include "nb_common.h"
#include "nb_dispatch.h"

// Let Kernel be launched with `bytes` of dynamic LDS (more than 64 KiB needs
// the opt-in): one call of the runtime whenever a launch asks for more than
// this kernel was granted before.  What was granted is remembered per process,
// not per device.
template <auto Kernel>
int nb_allow_lds(size_t bytes) {
  static size_t allowed = 0;
  if (bytes > allowed) {
    const hipError_t e = hipFuncSetAttribute(
        (const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)bytes);
    if (e != hipSuccess) {
      nb_set_error("hipFuncSetAttribute(%zu bytes LDS) failed: %s", bytes,
                   hipGetErrorString(e));
      return NB_ERR_HIP;
    }
    allowed = bytes;
  }
  return NB_OK;
}

// The launch shape of the row-streaming kernels (nb_poisson_kernel,
// nb_rowprod_kernel): L lanes share a row, a lane group walks R rows and U
// column blocks of L per step, workgroups of 256 lanes.
template <int L_, int R_, int U_>
struct nb_stream_shape {
  static constexpr int L = L_, R = R_, U = U_;
  static unsigned grid(long long n) {            // workgroups for n rows
    constexpr long long rows = (256 / L) * R;    // of a workgroup per step
    const long long b = (n + rows - 1) / rows;
    return (unsigned)(b > 8192 ? 8192 : b);
  }
};

// launch(shape) with the shape of P = n_data.  It is a function of P alone (a
// row's bits depend on it): short rows put their independent work into
// several rows per lane, long rows into column blocks of a whole wavefront.
// device.stream_launch_shape repeats it for the tests' error budgets.
template <class F>
int nb_stream_dispatch(int n_data, F launch) {
  if (n_data <= 32) return launch(nb_stream_shape<16, 4, 1>());
  if (n_data <= 512) return launch(nb_stream_shape<16, 2, 2>());
  return launch(nb_stream_shape<64, 1, 4>());
}

bool nb_eval_fast_eligible(int n_dim, int K, int M, int E, bool sample);
int nb_launch_eval_fast(const double* blob_dev, int n_dim, bool sample, int m,
                        int recentre, const double* x, const long long* idx,
                        long long n,
                        unsigned char* out_u8, double* out_f64,
                        unsigned long long seed, unsigned long long offset,
                        hipStream_t stream);
int nb_launch_cand(int dt, int n_dim, const double* const* blobs_dev,
                   const int* group_base_dev, int nb, int n_groups, int b_off,
                   int g_off, int accumulate, int mode, const double* x,
                   long long n, unsigned char* st, int* first, int* work,
                   unsigned long long seed, unsigned long long offset,
                   int** dense_out, int** totals_out, long long* n_pad_out,
                   hipStream_t stream);
long long nb_cand_work_bytes(int dt, int mode, long long n, int n_groups);
int nb_launch_eval_fast_batch(const double* blob0_dev, int n_dim, int recentre,
                              const double* x, const void* groups_dev,
                              int n_groups, const int* totals_dev,
                              const int* dense_dev, long long n_pad,
                              long long n_upper, int out_mode,
                              unsigned char* st, int* first,
                              hipStream_t stream);
// count = 0: out_f64[2 i] = r2 against neural bound 0, out_f64[2 i + 1] = 0;
// count = 1: out_u8[i] = outer members containing row i (nb_geom.hip)
int nb_launch_geom(const double* blob_dev, int dt, int count, const double* x,
                   long long n, double* out_f64, unsigned char* out_u8,
                   hipStream_t stream);
// optional device counters of the bound evaluation (nb_api.hip): [0] outer
// member, [1] neural ellipsoid, [2] emulator point evaluations; null = off
void nb_eval_set_counters(unsigned long long* dev);
unsigned long long* nb_eval_counters();
int nb_launch_draw(const double* blob_dev, int n_dim, unsigned long long seed,
                   unsigned long long offset, long long n, double* x_out,
                   hipStream_t stream);
int nb_launch_transform(const double* ell_block, int dt, int n_dim,
                        const double* x, long long n, double* y,
                        hipStream_t stream);
int nb_launch_standardize(const double* x, long long n, int d, double* mean,
                          double* scale, double* out, hipStream_t stream);
int nb_launch_prior_table(const double* u, long long n, int d,
                          const double* par, const unsigned char* kind,
                          int n_keys, const int* key_column,
                          const double* key_value, int column_major,
                          int level, double* out, hipStream_t stream);
int nb_launch_ell_stream(const double* cvec, const double* binv, int n_dim,
                         const double* x, long long n, unsigned char* mask,
                         hipStream_t stream);
int nb_launch_mixture(const double* blob, int n_dim, int n_comp,
                      const double* x, long long n, double* out, int* label,
                      hipStream_t stream);
int nb_launch_chi2(const double* blob, int n_data, const double* model,
                   long long ld, long long n, double log_norm, double* out,
                   hipStream_t stream);
int nb_launch_chi2_diag(const double* blob, int n_data, const double* model,
                        long long ld, long long n, double log_norm,
                        double* out, hipStream_t stream);
int nb_launch_poisson(const double* tab, int n_data, const double* model,
                      long long ld, long long n, double log_const,
                      double* out, hipStream_t stream);
int nb_launch_noise(const double* tab, int n_data, int mode,
                    const double* model, long long ld, const double* noise,
                    long long ld_noise, long long n, double log_norm,
                    double* out, hipStream_t stream);
int nb_launch_outlier(const double* tab, int n_data, const double* model,
                      long long ld, const double* mix, long long ld_mix,
                      long long n, double log_norm, double* out,
                      hipStream_t stream);
int nb_launch_gp(const double* tab, int n_data, int kernel, int mode,
                 const double* model, long long ld, const double* cov,
                 long long ld_cov, long long n, double log_norm, double* out,
                 hipStream_t stream);
int nb_launch_gps(const double* tab, int n_data, const nb_gps_plan& plan,
                  const double* model, long long ld, const double* hyper,
                  long long ld_hyper, long long n, double log_norm,
                  double* out, hipStream_t stream);
int nb_launch_fold_poisson(const double* blob, int n_data, int n_src,
                           const double* src, long long ld, long long n,
                           double log_const, double* out, hipStream_t stream);
