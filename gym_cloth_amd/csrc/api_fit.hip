// api_fit.hip -- the supervised trainer of the handle's shared network: the device-resident dataset, the loss and its gradient over a minibatch, the optimizer steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "api_handle.hpp"
#include "cloth_policy_fit.hpp"
#include "cloth_policy_mlp.hpp"

static_assert(FIT_MAX_BATCH == CLOTHHIP_FIT_MAX_BATCH, "the batch cap of the header and of the kernels");
static_assert(sizeof(ClothFitParams) == 24, "ClothFitParams is six floats");

// ---- the dataset (clothhip.h: clothhip_fit_data_*) ------------------------------------------------------------------------------------
extern "C" int clothhip_fit_data_append(clothhip_handle *h, const float *obs_rows, const double *labels, int64_t n) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (n < 0) return fail(CLOTHHIP_EINVAL, "n < 0");
    if (n == 0) return 0;
    if (!obs_rows || !labels) return fail(CLOTHHIP_EINVAL, "NULL argument");
    auto &f = h->fit;
    const size_t row = (size_t)3 * h->P;
    if (f.n + n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "%lld + %lld rows: a minibatch names its rows by int32", (long long)f.n, (long long)n);
    for (size_t i = 0; i < (size_t)n * row; i++)
        if (!std::isfinite(obs_rows[i])) return fail(CLOTHHIP_EINVAL, "obs_rows[%zu][%zu] is not finite", i / row, i % row);
    std::vector<float> lab;
    try { lab.resize((size_t)n * 4); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld labels)", (long long)n); }
    for (size_t i = 0; i < (size_t)n * 4; i++) {
        lab[i] = (float)labels[i];
        if (!std::isfinite(lab[i])) return fail(CLOTHHIP_EINVAL, "labels[%zu][%zu] is not a finite float (a slot that did not run? pass the rows that ran)", i / 4, i % 4);
    }
    HIPCHECK(hipSetDevice(h->device));
    if (f.n + n > f.cap) {      // grow geometrically into new tables, keep the rows (Buffer::reserve would not), swap them in
        const int64_t cap = std::max<int64_t>(std::max<int64_t>(f.n + n, 2 * f.cap), 64);
        Buffer<float> obs, lb;
        if (int rc = obs.reserve((size_t)cap * row * 4)) return rc;
        if (int rc = lb.reserve((size_t)cap * 4 * 4)) return rc;
        if (f.n > 0) {
            HIPCHECK(hipMemcpyAsync(obs, f.d_obs, (size_t)f.n * row * 4, hipMemcpyDeviceToDevice, h->stream));
            HIPCHECK(hipMemcpyAsync(lb, f.d_lab, (size_t)f.n * 4 * 4, hipMemcpyDeviceToDevice, h->stream));
            HIPCHECK(hipStreamSynchronize(h->stream));
        }
        f.d_obs = std::move(obs); f.d_lab = std::move(lb); f.cap = cap;
    }
    HIPCHECK(hipMemcpyAsync(f.d_obs + (size_t)f.n * row, obs_rows, (size_t)n * row * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_lab + (size_t)f.n * 4, lab.data(), (size_t)n * 4 * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // the host tables are never retained; only now do the rows count
    f.n += n;
    return 0;
}

extern "C" int clothhip_fit_data_clear(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit.n = 0;
    return 0;
}

extern "C" int clothhip_fit_data_size(clothhip_handle *h, int64_t *n) {
    if (!h || !n) return fail(CLOTHHIP_EINVAL, "NULL argument");
    *n = h->fit.n;
    return 0;
}

// ---- the gradient (cloth_policy_fit.hpp has the definition and the order) ---------------------------------------------------------------
// what both entries refuse before anything is touched
static int check_fit(const clothhip_handle *h, const int32_t *idx, int64_t n_idx, int32_t B) {
    if (int rc = check_idle(h)) return rc;
    if (h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: the fit trains the ONE shared network of clothhip_set_policy_mlp");
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    if (h->fit.n < 1) return fail(CLOTHHIP_ESTATE, "the dataset is empty: call clothhip_fit_data_append first");
    if (B < 1 || B > FIT_MAX_BATCH) return fail(CLOTHHIP_EINVAL, "B = %d outside [1, %d]", B, FIT_MAX_BATCH);
    if (!idx && n_idx > 0) return fail(CLOTHHIP_EINVAL, "idx is NULL");
    for (int64_t i = 0; i < n_idx; i++)
        if (idx[i] < 0 || idx[i] >= h->fit.n) return fail(CLOTHHIP_EINVAL, "idx[%lld] = %d outside [0, %lld)", (long long)i, idx[i], (long long)h->fit.n);
    return 0;
}

template <bool A_KC, bool B_KC, int EPI, bool ROWS> static void launch_gemm(hipStream_t s, const FitGemmArgs &a) {
    const dim3 grid((unsigned)((a.N + FIT_TILE - 1) / FIT_TILE), (unsigned)((a.M + FIT_TILE - 1) / FIT_TILE), (unsigned)((a.K + a.k_chunk - 1) / a.k_chunk));
    hipLaunchKernelGGL((k_fit_gemm<A_KC, B_KC, EPI, ROWS>), grid, dim3(FIT_THREADS), 0, s, a);
}

// this step's scratch for minibatches of B rows; the widest layer and the largest weight matrix size the shared tables
static int reserve_fit(clothhip_handle *h, int32_t B) {
    const MlpDesc &D = h->pol.mlp;
    size_t act = (size_t)B * MLP_OUT, maxw = MLP_OUT, maxmat = 0;
    for (int l = 0; l < D.n_layers; l++) {
        if (l + 1 < D.n_layers) act += (size_t)B * D.widths[l + 1];
        maxw = std::max<size_t>(maxw, D.widths[l + 1]);
        maxmat = std::max<size_t>(maxmat, (size_t)D.widths[l + 1] * D.widths[l]);
    }
    const size_t n_split = ((size_t)B + FIT_SPLIT_ROWS - 1) / FIT_SPLIT_ROWS;
    if (int rc = h->fit.d_act.reserve(act * 4)) return rc;
    if (int rc = h->fit.d_dz.reserve(2 * (size_t)B * maxw * 4)) return rc;
    if (n_split > 1) if (int rc = h->fit.d_part.reserve(n_split * maxmat * 4)) return rc;
    return h->fit.d_grad.reserve(h->pol.mlp_n_params * 4);
}

// enqueue loss and gradient of the present weights over rows d_idx[0 .. B): h->fit.d_grad (blob layout), *d_loss
static int enqueue_grad(clothhip_handle *h, const int32_t *d_idx, int32_t B, double *d_loss) {
    const MlpDesc &D = h->pol.mlp;
    const int L = D.n_layers;
    auto &f = h->fit;
    const float *W[MLP_MAX_LAYERS], *H[MLP_MAX_LAYERS];      // H[l]: layer l's output; H[L - 1] = y
    float *act = f.d_act, *gW[MLP_MAX_LAYERS];
    size_t maxw = MLP_OUT;
    {
        const float *w = D.params;
        float *g = f.d_grad, *a = act;
        for (int l = 0; l < L; l++) {
            W[l] = w; gW[l] = g; H[l] = a;
            const size_t n = (size_t)D.widths[l + 1] * D.widths[l] + D.widths[l + 1];
            w += n; g += n; a += (size_t)B * D.widths[l + 1];
            maxw = std::max<size_t>(maxw, D.widths[l + 1]);
        }
    }
    float *dz[2] = {f.d_dz, f.d_dz + (size_t)B * maxw};
    // forward
    for (int l = 0; l < L; l++) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        FitGemmArgs a = {};
        a.A = l ? H[l - 1] : (const float *)f.d_obs; a.lda = n_in; a.rows = l ? nullptr : d_idx;
        a.B = W[l]; a.ldb = n_in; a.bias = W[l] + (size_t)n_out * n_in;
        a.C = const_cast<float *>(H[l]); a.ldc = n_out;
        a.M = B; a.N = n_out; a.K = n_in; a.k_chunk = n_in;
        if (l == 0 && l + 1 < L) launch_gemm<true, true, FIT_EPI_BIAS_RELU, true>(h->stream, a);
        else if (l == 0) launch_gemm<true, true, FIT_EPI_BIAS, true>(h->stream, a);
        else if (l + 1 < L) launch_gemm<true, true, FIT_EPI_BIAS_RELU, false>(h->stream, a);
        else launch_gemm<true, true, FIT_EPI_BIAS, false>(h->stream, a);
        HIPCHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_fit_loss, dim3(1), dim3(256), 0, h->stream, H[L - 1], (const float *)f.d_lab, d_idx, B, dz[(L - 1) & 1], d_loss);
    HIPCHECK(hipGetLastError());
    // backward
    const int n_split = (B + FIT_SPLIT_ROWS - 1) / FIT_SPLIT_ROWS;
    for (int l = L - 1; l >= 0; l--) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        const float *dzl = dz[l & 1];
        FitGemmArgs a = {};
        a.A = dzl; a.lda = n_out;
        a.B = l ? H[l - 1] : (const float *)f.d_obs; a.ldb = n_in; a.rows = l ? nullptr : d_idx;
        a.C = n_split > 1 ? (float *)f.d_part : gW[l]; a.ldc = n_in; a.c_slab = (int64_t)n_out * n_in;
        a.M = n_out; a.N = n_in; a.K = B; a.k_chunk = FIT_SPLIT_ROWS;
        if (l == 0) launch_gemm<false, false, FIT_EPI_NONE, true>(h->stream, a);
        else launch_gemm<false, false, FIT_EPI_NONE, false>(h->stream, a);
        HIPCHECK(hipGetLastError());
        if (n_split > 1) {
            const int64_t n = (int64_t)n_out * n_in;
            hipLaunchKernelGGL(k_fit_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float *)f.d_part, n, n_split, gW[l], n);
            HIPCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_fit_colsum, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, h->stream, dzl, B, n_out, gW[l] + (size_t)n_out * n_in);
        HIPCHECK(hipGetLastError());
        if (l > 0) {
            FitGemmArgs b = {};
            b.A = dzl; b.lda = n_out;
            b.B = W[l]; b.ldb = n_in;
            b.mask = H[l - 1];
            b.C = dz[(l - 1) & 1]; b.ldc = n_in;
            b.M = B; b.N = n_in; b.K = n_out; b.k_chunk = n_out;
            launch_gemm<true, false, FIT_EPI_MASK, false>(h->stream, b);
            HIPCHECK(hipGetLastError());
        }
    }
    return 0;
}

extern "C" int clothhip_policy_fit_grad(clothhip_handle *h, const int32_t *idx, int32_t B, float *grad_out, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit(h, idx, B > 0 ? B : 0, B)) return rc;
    if (!idx) return fail(CLOTHHIP_EINVAL, "idx is NULL");
    auto &f = h->fit;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = reserve_fit(h, B)) return rc;
    if (int rc = f.d_idx.reserve((size_t)B * 4)) return rc;
    if (int rc = f.d_loss.reserve(8)) return rc;
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    if (int rc = enqueue_grad(h, f.d_idx, B, f.d_loss)) return rc;
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    if (grad_out) HIPCHECK(hipMemcpyAsync(grad_out, f.d_grad, h->pol.mlp_n_params * 4, hipMemcpyDeviceToHost, h->stream));
    if (loss_out) HIPCHECK(hipMemcpyAsync(loss_out, f.d_loss, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the optimizer ----------------------------------------------------------------------------------------------------------------------
static bool hyper_ok(float v) { return std::isfinite(v) && v >= 0.0f; }

extern "C" int clothhip_policy_fit(clothhip_handle *h, const ClothFitParams *p, const int32_t *idx, int32_t n_steps, int32_t B, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit(h, idx, B > 0 ? (int64_t)n_steps * B : 0, B)) return rc;
    const bool adam = p->optimizer == (float)CLOTHHIP_FIT_ADAM;
    if (!adam && p->optimizer != (float)CLOTHHIP_FIT_SGD) return fail(CLOTHHIP_EINVAL, "unknown optimizer %g (CLOTHHIP_FIT_ADAM or CLOTHHIP_FIT_SGD)", (double)p->optimizer);
    if (!hyper_ok(p->lr) || !hyper_ok(p->eps) || !hyper_ok(p->momentum) || !hyper_ok(p->beta1) || !hyper_ok(p->beta2))
        return fail(CLOTHHIP_EINVAL, "a hyper-parameter is negative or not finite (lr %g, beta1 %g, beta2 %g, eps %g, momentum %g)", (double)p->lr,
                    (double)p->beta1, (double)p->beta2, (double)p->eps, (double)p->momentum);
    if (p->beta1 >= 1.0f || p->beta2 >= 1.0f) return fail(CLOTHHIP_EINVAL, "beta1 %g, beta2 %g: both lie in [0, 1)", (double)p->beta1, (double)p->beta2);
    if (n_steps == 0) return 0;
    auto &f = h->fit;
    const size_t n = h->pol.mlp_n_params;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = reserve_fit(h, B)) return rc;
    if (int rc = f.d_idx.reserve((size_t)n_steps * B * 4)) return rc;
    if (int rc = f.d_loss.reserve((size_t)n_steps * 8)) return rc;
    if (int rc = f.d_m.reserve(n * 4)) return rc;
    if (int rc = f.d_v.reserve(n * 4)) return rc;
    // from here on the call goes through (but for a failure of the runtime itself)
    if (f.opt_zero) {
        HIPCHECK(hipMemsetAsync(f.d_m, 0, n * 4, h->stream));
        HIPCHECK(hipMemsetAsync(f.d_v, 0, n * 4, h->stream));
        f.opt_zero = false;
    }
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)n_steps * B * 4, hipMemcpyHostToDevice, h->stream));
    float *theta = h->pol.d_mlp;
    const double b1 = (double)p->beta1, b2 = (double)p->beta2;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int s = 0; s < n_steps; s++) {
        if (int rc = enqueue_grad(h, f.d_idx + (size_t)s * B, B, f.d_loss + s)) return rc;
        const double t = (double)(++f.opt_t);
        if (adam) {
            const double a_t = (double)p->lr * std::sqrt(1.0 - std::pow(b2, t)) / (1.0 - std::pow(b1, t));
            hipLaunchKernelGGL(k_fit_adam, dim3(blocks), dim3(256), 0, h->stream, theta, (float *)f.d_m, (float *)f.d_v, (const float *)f.d_grad, (int64_t)n,
                               (float)a_t, p->beta1, (float)(1.0 - b1), p->beta2, (float)(1.0 - b2), p->eps);
        } else {
            hipLaunchKernelGGL(k_fit_sgd, dim3(blocks), dim3(256), 0, h->stream, theta, (float *)f.d_m, (const float *)f.d_grad, (int64_t)n, p->lr, p->momentum);
        }
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    if (loss_out) HIPCHECK(hipMemcpyAsync(loss_out, f.d_loss, (size_t)n_steps * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_fit_reset(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit_forget();
    return 0;
}
