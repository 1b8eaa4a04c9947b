// api_policy.hip -- a learned policy on the handle: the network, a population of networks, their stand-alone evaluation; the analytic experts' stand-alone labelling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "api_handle.hpp"
#include "cloth_policy_eval.hpp"
#include "cloth_policy_label.hpp"
#include "cloth_policy_noise.hpp"
#include "cloth_policy_population.hpp"

// ---- a learned policy: the handle's network (cloth_policy_mlp.hpp) ----------------------------------------------------------------------
// the shape rules of every entry that takes a network
// (n_act: the action components behind the observation in a row of the network's input -- 4 for the Q network, else none)
static int check_mlp_shape(const clothhip_handle *h, int32_t n_layers, const int32_t *widths, int32_t n_out = MLP_OUT, int32_t n_act = 0) {
    if (n_layers < 1 || n_layers > MLP_MAX_LAYERS) return fail(CLOTHHIP_EINVAL, "n_layers %d outside [0, %d]", n_layers, MLP_MAX_LAYERS);
    if (!widths) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_act && widths[0] != 3 * h->P + n_act)
        return fail(CLOTHHIP_EINVAL, "the network's input width is %d, the '1d' observation and an action have %d values", widths[0], 3 * h->P + n_act);
    if (!n_act && widths[0] != 3 * h->P) return fail(CLOTHHIP_EINVAL, "the network's input width is %d, the '1d' observation has %d values", widths[0], 3 * h->P);
    if (widths[n_layers] != n_out)
        return fail(CLOTHHIP_EINVAL, n_out == MLP_OUT ? "the network's output width is %d, an action has %d values" : "the network's output width is %d, a value is %d number", widths[n_layers], n_out);
    for (int l = 1; l < n_layers; l++)
        if (widths[l] < 1 || widths[l] > MLP_MAX_WIDTH) return fail(CLOTHHIP_EINVAL, "hidden width %d (layer %d) outside [1, %d]", widths[l], l, MLP_MAX_WIDTH);
    return 0;
}
static int check_members(const int32_t *member, int64_t n, int64_t rows, const char *what) {
    if (!member) return fail(CLOTHHIP_EINVAL, "%s is NULL", what);
    for (int64_t e = 0; e < n; e++)
        if (member[e] < 0 || member[e] >= rows) return fail(CLOTHHIP_EINVAL, "%s[%lld] = %d outside [0, %lld)", what, (long long)e, member[e], (long long)rows);
    return 0;
}
// the handle without a network of either kind (the memory stays with the handle for the next one); the trainer's moments belonged to the
// old one, and so did DDPG's target policy
static void drop_network(clothhip_handle *h) {
    h->fit.opt_policy.forget(); h->pol.mlp = MlpDesc{}; h->pol.pop_rows = 0; h->pol.mlp_n_params = 0; h->pol.pop_generated = false;
    h->tgt.policy_valid = false;
}
static MlpDesc mlp_desc(int32_t n_layers, const int32_t *widths, const float *params, const int32_t *member, size_t stride) {
    MlpDesc d = {};
    d.n_layers = n_layers;
    for (int l = 0; l <= n_layers; l++) d.widths[l] = widths[l];
    d.params = params; d.member = member; d.stride = (int64_t)stride;
    return d;
}

extern "C" int clothhip_set_policy_mlp(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (n_layers == 0) { drop_network(h); return 0; }
    if (int rc = check_mlp_shape(h, n_layers, widths)) return rc;
    if (!params) return fail(CLOTHHIP_EINVAL, "NULL argument");
    const size_t need = mlp_param_count(n_layers, widths);
    if (n_params != need) return fail(CLOTHHIP_EINVAL, "n_params = %zu, these widths hold %zu parameters", n_params, need);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));      // nothing in flight reads the blob reserve() may free
    drop_network(h);                                // from here on the old network is gone: a failure below leaves the handle without one
    if (int rc = h->pol.d_mlp.reserve(need * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->pol.d_mlp, params, need * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // the host blob is never retained
    h->pol.mlp = mlp_desc(n_layers, widths, h->pol.d_mlp, nullptr, 0);
    h->pol.mlp_n_params = need;
    return 0;
}

// ---- the log-sigma head (clothhip.h: PPO WITH A LEARNED SIGMA): four floats beside the blob, which no network entry above touches ---------
extern "C" int clothhip_set_policy_log_sigma(clothhip_handle *h, const float *ls) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (!ls) { h->pol.has_log_sigma = false; h->fit.opt_sigma.forget(); return 0; }
    for (int k = 0; k < MLP_OUT; k++)
        if (!std::isfinite(ls[k]) || std::fabs(ls[k]) > 10.0f) return fail(CLOTHHIP_EINVAL, "ls[%d] = %g: a log sigma is finite and lies in [-10, 10]", k, (double)ls[k]);
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = h->pol.d_log_sigma.reserve(MLP_OUT * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->pol.d_log_sigma, ls, MLP_OUT * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // the host values are never retained
    h->pol.has_log_sigma = true;
    h->fit.opt_sigma.forget();                      // the head's moments belonged to the old values; the blob's optimizer is not touched
    return 0;
}

extern "C" int clothhip_get_policy_log_sigma(clothhip_handle *h, float *out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (!h->pol.has_log_sigma) return fail(CLOTHHIP_ESTATE, "no log-sigma head on this handle: call clothhip_set_policy_log_sigma first");
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(out, h->pol.d_log_sigma, MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the exploration noise (clothhip.h: EXPLORATION NOISE ON THE DEVICE; cloth_policy_noise.hpp): the handle's table, filled on its stream --
extern "C" int clothhip_policy_noise_fill(clothhip_handle *h, uint64_t seed, int32_t T, const int64_t *slot_base, const double *sigma,
                                          int32_t sigma_rows, void **d_noise) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;          // (that launch may be reading the table)
    if (T < 1) return fail(CLOTHHIP_EINVAL, "T = %d: a table has at least one slot", T);
    const int64_t n = (int64_t)T * h->E;
    if (n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "T * E = %lld slots: more than 2^31 - 1", (long long)n);
    const bool head = !sigma;
    if (head && sigma_rows != 0) return fail(CLOTHHIP_EINVAL, "sigma_rows = %d without a sigma table (0: the handle's log-sigma head)", sigma_rows);
    if (!head && sigma_rows != 1 && sigma_rows != h->E)
        return fail(CLOTHHIP_EINVAL, "sigma_rows = %d: 1 (one sigma[4] for all envs) or %d (one per env)", sigma_rows, h->E);
    for (int64_t i = 0; !head && i < (int64_t)sigma_rows * MLP_OUT; i++)
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return fail(CLOTHHIP_EINVAL, "sigma[%lld][%d] = %g: a sigma is finite and not negative", (long long)(i / MLP_OUT), (int)(i % MLP_OUT), sigma[i]);
    if (head && !h->pol.has_log_sigma) return fail(CLOTHHIP_ESTATE, "no log-sigma head on this handle: call clothhip_set_policy_log_sigma first, or pass sigma");
    for (int e = 0; slot_base && e < h->E; e++)
        if (slot_base[e] < 0 || slot_base[e] > INT64_MAX - T) return fail(CLOTHHIP_EINVAL, "slot_base[%d] = %lld: a slot number is not negative (and slot_base + T fits 63 bits)", e, (long long)slot_base[e]);
    HIPCHECK(hipSetDevice(h->device));
    h->pol.noise_T = 0;                             // from here on the old table is gone: a failure below leaves the handle without one
    if (int rc = h->pol.d_noise.reserve((size_t)n * MLP_OUT * 8)) return rc;
    PolicyNoiseArgs a;
    memset(&a, 0, sizeof(a));
    a.out = h->pol.d_noise; a.seed = seed; a.n = n; a.E = h->E; a.sigma_rows = sigma_rows;
    if (head) a.log_sigma = h->pol.d_log_sigma;
    else {
        if (int rc = h->pol.d_noise_sigma.reserve((size_t)sigma_rows * MLP_OUT * 8)) return rc;
        HIPCHECK(hipMemcpyAsync(h->pol.d_noise_sigma, sigma, (size_t)sigma_rows * MLP_OUT * 8, hipMemcpyHostToDevice, h->stream));
        a.sigma = h->pol.d_noise_sigma;
    }
    if (slot_base) {
        if (int rc = h->pol.d_noise_base.reserve((size_t)h->E * 8)) return rc;
        HIPCHECK(hipMemcpyAsync(h->pol.d_noise_base, slot_base, (size_t)h->E * 8, hipMemcpyHostToDevice, h->stream));
        a.slot_base = h->pol.d_noise_base;
    }
    if (!head || slot_base) HIPCHECK(hipStreamSynchronize(h->stream));      // the host tables are never retained (the head route uploads nothing and waits for nothing)
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_policy_noise_fill, dim3((unsigned)((n + NOISE_THREADS - 1) / NOISE_THREADS)), dim3(NOISE_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;                          // clothhip_last_kernel_ms: this kernel
    h->pol.noise_T = T;
    if (d_noise) *d_noise = (double *)h->pol.d_noise;
    return 0;
}

extern "C" int clothhip_policy_noise_get(clothhip_handle *h, int32_t T, double *out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.noise_T < 1) return fail(CLOTHHIP_ESTATE, "no noise table on this handle: call clothhip_policy_noise_fill first");
    if (T != h->pol.noise_T) return fail(CLOTHHIP_EINVAL, "T = %d, the last clothhip_policy_noise_fill made %d slots", T, h->pol.noise_T);
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(out, h->pol.d_noise, (size_t)T * h->E * MLP_OUT * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the value network (clothhip.h: ACTOR-CRITIC FROM REWARD): the policy's shape rules with ONE output; the handle's other network ------------
extern "C" int clothhip_set_value_mlp(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    auto drop = [h] { h->fit.opt_value.forget(); h->val.mlp = MlpDesc{}; h->val.n_params = 0; };
    if (n_layers == 0) { drop(); return 0; }
    if (int rc = check_mlp_shape(h, n_layers, widths, 1)) return rc;
    if (!params) return fail(CLOTHHIP_EINVAL, "NULL argument");
    const size_t need = mlp_param_count(n_layers, widths);
    if (n_params != need) return fail(CLOTHHIP_EINVAL, "n_params = %zu, these widths hold %zu parameters", n_params, need);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    drop();                                         // as clothhip_set_policy_mlp: a failure below leaves the handle without a value network
    if (int rc = h->val.d_mlp.reserve(need * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->val.d_mlp, params, need * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->val.mlp = mlp_desc(n_layers, widths, h->val.d_mlp, nullptr, 0);
    h->val.n_params = need;
    return 0;
}

extern "C" int clothhip_get_value_mlp(clothhip_handle *h, float *out, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->val.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no value network on this handle: call clothhip_set_value_mlp first");
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    if (n_params != h->val.n_params) return fail(CLOTHHIP_EINVAL, "n_params = %zu, the value network holds %zu parameters", n_params, h->val.n_params);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(out, h->val.d_mlp, n_params * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- DDPG's networks (clothhip.h: DDPG ON THE DEVICE): the Q network over (observation, action), and the target copies ---------------------
extern "C" int clothhip_set_q_mlp(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    auto drop = [h] { h->fit.opt_q.forget(); h->fit.ddpg_B = 0; h->qnet.mlp = MlpDesc{}; h->qnet.n_params = 0; h->tgt.q_valid = false; };
    if (n_layers == 0) { drop(); return 0; }
    if (int rc = check_mlp_shape(h, n_layers, widths, 1, MLP_OUT)) return rc;
    if (!params) return fail(CLOTHHIP_EINVAL, "NULL argument");
    const size_t need = mlp_param_count(n_layers, widths);
    if (n_params != need) return fail(CLOTHHIP_EINVAL, "n_params = %zu, these widths hold %zu parameters", n_params, need);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    drop();                                         // as clothhip_set_value_mlp: a failure below leaves the handle without a Q network
    if (int rc = h->qnet.d_mlp.reserve(need * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->qnet.d_mlp, params, need * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->qnet.mlp = mlp_desc(n_layers, widths, h->qnet.d_mlp, nullptr, 0);
    h->qnet.n_params = need;
    return 0;
}

extern "C" int clothhip_get_q_mlp(clothhip_handle *h, float *out, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->qnet.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no Q network on this handle: call clothhip_set_q_mlp first");
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    if (n_params != h->qnet.n_params) return fail(CLOTHHIP_EINVAL, "n_params = %zu, the Q network holds %zu parameters", n_params, h->qnet.n_params);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(out, h->qnet.d_mlp, n_params * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_ddpg_sync_targets(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: DDPG trains the ONE shared network of clothhip_set_policy_mlp");
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    if (h->qnet.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no Q network on this handle: call clothhip_set_q_mlp first");
    HIPCHECK(hipSetDevice(h->device));
    h->tgt.policy_valid = h->tgt.q_valid = false;   // a failure below leaves the handle without targets
    if (int rc = h->tgt.d_policy.reserve(h->pol.mlp_n_params * 4)) return rc;
    if (int rc = h->tgt.d_q.reserve(h->qnet.n_params * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->tgt.d_policy, h->pol.d_mlp, h->pol.mlp_n_params * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->tgt.d_q, h->qnet.d_mlp, h->qnet.n_params * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->tgt.policy_valid = h->tgt.q_valid = true;
    return 0;
}

// the targets from the host (a checkpoint's): either blob may be NULL, which leaves that target as it is
extern "C" int clothhip_ddpg_set_targets(clothhip_handle *h, const float *policy, const float *q) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: DDPG trains the ONE shared network of clothhip_set_policy_mlp");
    if (policy && h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first (the target policy has its shape)");
    if (q && h->qnet.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no Q network on this handle: call clothhip_set_q_mlp first (the target Q network has its shape)");
    HIPCHECK(hipSetDevice(h->device));
    if (policy) {
        h->tgt.policy_valid = false;
        if (int rc = h->tgt.d_policy.reserve(h->pol.mlp_n_params * 4)) return rc;
        HIPCHECK(hipMemcpyAsync(h->tgt.d_policy, policy, h->pol.mlp_n_params * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (q) {
        h->tgt.q_valid = false;
        if (int rc = h->tgt.d_q.reserve(h->qnet.n_params * 4)) return rc;
        HIPCHECK(hipMemcpyAsync(h->tgt.d_q, q, h->qnet.n_params * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));      // the host blobs are never retained
    if (policy) h->tgt.policy_valid = true;
    if (q) h->tgt.q_valid = true;
    return 0;
}

extern "C" int clothhip_ddpg_get_targets(clothhip_handle *h, float *policy_out, float *q_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (policy_out && !h->tgt.policy_valid) return fail(CLOTHHIP_ESTATE, "no target policy on this handle: call clothhip_ddpg_sync_targets first");
    if (q_out && !h->tgt.q_valid) return fail(CLOTHHIP_ESTATE, "no target Q network on this handle: call clothhip_ddpg_sync_targets first");
    HIPCHECK(hipSetDevice(h->device));
    if (policy_out) HIPCHECK(hipMemcpyAsync(policy_out, h->tgt.d_policy, h->pol.mlp_n_params * 4, hipMemcpyDeviceToHost, h->stream));
    if (q_out) HIPCHECK(hipMemcpyAsync(q_out, h->tgt.d_q, h->qnet.n_params * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- a population: one network per env slot (cloth_policy_mlp.hpp MlpDesc::member, cloth_policy_population.hpp) ----------------------------------
static int upload_members(clothhip_handle *h, const int32_t *member) {
    if (int rc = h->pol.d_member.reserve((size_t)h->E * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->pol.d_member, member, (size_t)h->E * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_set_policy_population(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, int32_t G,
                                              const int32_t *member) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (n_layers == 0) { drop_network(h); return 0; }
    if (int rc = check_mlp_shape(h, n_layers, widths)) return rc;
    if (!params) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (G < 1) return fail(CLOTHHIP_EINVAL, "G = %d: a population has at least one network", G);
    if (int rc = check_members(member, h->E, G, "member")) return rc;
    const size_t n = mlp_param_count(n_layers, widths), stride = population_stride(n);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    drop_network(h);                                // as clothhip_set_policy_mlp: a failure below leaves the handle without a network
    if (int rc = h->pol.d_pop.reserve((size_t)G * stride * 4)) return rc;
    HIPCHECK(hipMemsetAsync(h->pol.d_pop, 0, (size_t)G * stride * 4, h->stream));      // the pad is zeros
    HIPCHECK(hipMemcpy2DAsync(h->pol.d_pop, stride * 4, params, n * 4, n * 4, (size_t)G, hipMemcpyHostToDevice, h->stream));
    if (int rc = upload_members(h, member)) return rc;
    h->pol.mlp = mlp_desc(n_layers, widths, h->pol.d_pop, h->pol.d_member, stride);
    h->pol.mlp_n_params = n; h->pol.pop_rows = G;
    return 0;
}

extern "C" int clothhip_set_policy_members(clothhip_handle *h, const int32_t *member) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.pop_rows < 1) return fail(CLOTHHIP_ESTATE, "no population on this handle: call clothhip_set_policy_population or clothhip_policy_population_perturb first");
    if (int rc = check_members(member, h->E, h->pol.pop_rows, "member")) return rc;
    HIPCHECK(hipSetDevice(h->device));
    return upload_members(h, member);
}

extern "C" int clothhip_get_policy_mlp(clothhip_handle *h, int64_t g, float *out, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle");
    const int64_t rows = h->pol.pop_rows ? h->pol.pop_rows : 1;
    if (g < 0 || g >= rows) return fail(CLOTHHIP_EINVAL, "g = %lld outside [0, %lld)", (long long)g, (long long)rows);
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    if (n_params != h->pol.mlp_n_params && !(h->pol.pop_rows && n_params == (size_t)h->pol.mlp.stride))
        return fail(CLOTHHIP_EINVAL, "n_params = %zu, the network holds %zu parameters", n_params, h->pol.mlp_n_params);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(out, h->pol.mlp.params + (size_t)g * (size_t)h->pol.mlp.stride, n_params * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_population_perturb(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *center, int32_t G,
                                                  float sigma, uint64_t seed, int32_t flags, const int32_t *member) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (int rc = check_mlp_shape(h, n_layers, widths)) return rc;
    if (!center) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (flags & ~CLOTHHIP_POP_ANTITHETIC) return fail(CLOTHHIP_EINVAL, "unknown flags 0x%x", flags);
    const bool anti = (flags & CLOTHHIP_POP_ANTITHETIC) != 0;
    if (G < 1 || G > POP_MAX_G) return fail(CLOTHHIP_EINVAL, "G = %d outside [1, %d]", G, POP_MAX_G);
    if (anti && (G & 1)) return fail(CLOTHHIP_EINVAL, "G = %d: antithetic perturbations come in pairs, G must be even", G);
    if (!std::isfinite(sigma)) return fail(CLOTHHIP_EINVAL, "sigma is not finite");
    if (int rc = check_members(member, h->E, (int64_t)G + 1, "member")) return rc;
    const size_t n = mlp_param_count(n_layers, widths), stride = population_stride(n), rows = (size_t)G + 1;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    drop_network(h);
    if (int rc = h->pol.d_pop.reserve(rows * stride * 4)) return rc;
    if (int rc = h->pol.d_pop_center.reserve(n * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->pol.d_pop_center, center, n * 4, hipMemcpyHostToDevice, h->stream));
    PopulationPerturbArgs a;
    memset(&a, 0, sizeof(a));
    a.center = h->pol.d_pop_center; a.rows = h->pol.d_pop; a.n_params = n; a.stride = stride; a.seed = seed;
    a.K = anti ? G / 2 : G; a.antithetic = anti ? 1 : 0; a.sigma = sigma;
    const size_t per_row = (stride / 4 + POP_THREADS - 1) / POP_THREADS;
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_population_perturb, dim3((unsigned)per_row, (unsigned)(a.K + 1)), dim3(POP_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;                                  // clothhip_last_kernel_ms: this kernel
    if (int rc = upload_members(h, member)) return rc;      // (synchronises: the host centre is never retained)
    h->pol.mlp = mlp_desc(n_layers, widths, h->pol.d_pop, h->pol.d_member, stride);
    h->pol.mlp_n_params = n; h->pol.pop_rows = (int64_t)rows;
    h->pol.pop_generated = true; h->pol.pop_seed = seed; h->pol.pop_sigma = sigma; h->pol.pop_flags = flags;
    return 0;
}

extern "C" int clothhip_policy_population_combine(clothhip_handle *h, const float *coef, int32_t K, float *out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.pop_rows < 1) return fail(CLOTHHIP_ESTATE, "no population on this handle: call clothhip_policy_population_perturb first");
    if (!h->pol.pop_generated) return fail(CLOTHHIP_ESTATE, "this population was uploaded (clothhip_set_policy_population), not generated: there are no perturbations to sum");
    if (!coef || !out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    const int64_t G = h->pol.pop_rows - 1, want = (h->pol.pop_flags & CLOTHHIP_POP_ANTITHETIC) ? G / 2 : G;
    if (K != want) return fail(CLOTHHIP_EINVAL, "K = %d, this population has %lld perturbations", K, (long long)want);
    const size_t n = h->pol.mlp_n_params;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = h->pol.d_pop_coef.reserve((size_t)K * 4)) return rc;
    if (int rc = h->pol.d_pop_out.reserve(n * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->pol.d_pop_coef, coef, (size_t)K * 4, hipMemcpyHostToDevice, h->stream));
    PopulationCombineArgs a;
    memset(&a, 0, sizeof(a));
    a.coef = h->pol.d_pop_coef; a.out = h->pol.d_pop_out; a.n_params = n; a.seed = h->pol.pop_seed; a.K = K;
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_population_combine, dim3((unsigned)((n + POP_THREADS - 1) / POP_THREADS)), dim3(POP_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipMemcpyAsync(out, h->pol.d_pop_out, n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// rows per chunk: the uploaded rows of one chunk take at most 32 MB, whatever n is
static size_t policy_eval_chunk(int P) {
    const size_t c = ((size_t)32 << 20) / ((size_t)3 * P * 4);
    return c < 1 ? 1 : (c > 65536 ? 65536 : c);
}

// both evaluation entries; members == nullptr: every row under the shared network
static int policy_eval_rows(clothhip_handle *h, const float *obs_rows, int64_t n, const int32_t *members, double *actions_out) {
    if (n < 0) return fail(CLOTHHIP_EINVAL, "n < 0");
    if (!obs_rows && n != h->E) return fail(CLOTHHIP_EINVAL, "n = %lld, the handle's state holds %d cloths", (long long)n, h->E);
    if (!actions_out && n > 0) return fail(CLOTHHIP_EINVAL, "actions_out is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    if (!members && h->pol.pop_rows)
        return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: clothhip_policy_eval_members says which one evaluates a row");
    if (n == 0) return 0;
    if (members) if (int rc = check_members(members, n, h->pol.pop_rows ? h->pol.pop_rows : 1, "members")) return rc;
    HIPCHECK(hipSetDevice(h->device));
    const size_t row = (size_t)3 * h->P, chunk = policy_eval_chunk(h->P), cmax = (size_t)n < chunk ? (size_t)n : chunk;
    if (obs_rows) if (int rc = h->pol.d_pe_rows.reserve(cmax * row * 4)) return rc;
    if (int rc = h->pol.d_pe_out.reserve(cmax * MLP_OUT * 8)) return rc;
    if (members) if (int rc = h->pol.d_pe_mem.reserve(cmax * 4)) return rc;
    PolicyEvalArgs a;
    memset(&a, 0, sizeof(a));
    a.mlp = h->pol.mlp; a.P = h->P; a.Ppad = h->Ppad; a.out = h->pol.d_pe_out;
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const size_t m = (size_t)n - i0 < chunk ? (size_t)n - i0 : chunk;
        if (members) {
            HIPCHECK(hipMemcpyAsync(h->pol.d_pe_mem, members + i0, m * 4, hipMemcpyHostToDevice, h->stream));
            a.members = h->pol.d_pe_mem;
        }
        if (obs_rows) {
            HIPCHECK(hipMemcpyAsync(h->pol.d_pe_rows, obs_rows + i0 * row, m * row * 4, hipMemcpyHostToDevice, h->stream));
            a.rows = h->pol.d_pe_rows;
            hipLaunchKernelGGL(k_policy_eval<float>, dim3((unsigned)m), dim3(256), 0, h->stream, a);
        } else {
            by_precision(h, [&](auto t) {
                using T = decltype(t);
                a.pos = (const T *)h->d_pos + i0 * 3 * h->Ppad;
                hipLaunchKernelGGL(k_policy_eval<T>, dim3((unsigned)m), dim3(256), 0, h->stream, a);
            });
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(actions_out + i0 * MLP_OUT, h->pol.d_pe_out, m * MLP_OUT * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_eval(clothhip_handle *h, const float *obs_rows, int64_t n, double *actions_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    return policy_eval_rows(h, obs_rows, n, nullptr, actions_out);
}
extern "C" int clothhip_policy_eval_members(clothhip_handle *h, const float *obs_rows, int64_t n, const int32_t *members, double *actions_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!members && n > 0) return fail(CLOTHHIP_EINVAL, "members is NULL");
    return policy_eval_rows(h, obs_rows, n, members, actions_out);
}

// ---- the analytic experts on stored observations or on the present state (cloth_policy_label.hpp) -----------------------------------------
extern "C" int clothhip_policy_label(clothhip_handle *h, int32_t expert, int32_t clip_act_space, const float *obs_rows, int64_t n,
                                     const int32_t *side, const int32_t *choice, double *actions_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (expert != CLOTHHIP_POLICY_ORACLE_CORNER && expert != CLOTHHIP_POLICY_HIGHEST_POINT)
        return fail(CLOTHHIP_EINVAL, "unknown expert %d (CLOTHHIP_POLICY_ORACLE_CORNER or CLOTHHIP_POLICY_HIGHEST_POINT)", expert);
    if (n < 0) return fail(CLOTHHIP_EINVAL, "n < 0");
    if (!obs_rows && n != h->E) return fail(CLOTHHIP_EINVAL, "n = %lld, the handle's state holds %d cloths", (long long)n, h->E);
    if (expert == CLOTHHIP_POLICY_HIGHEST_POINT && !choice && n > 0) return fail(CLOTHHIP_EINVAL, "the highest-point expert needs choice[n]: which of the highest points per row");
    if (!actions_out && n > 0) return fail(CLOTHHIP_EINVAL, "actions_out is NULL");
    if (int rc = check_idle(h)) return rc;
    if (expert == CLOTHHIP_POLICY_ORACLE_CORNER && h->N != 25)
        return fail(CLOTHHIP_ESTATE, "the oracle-corner policy is defined for 25x25 cloths only (analytic.py:106)");
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(h->device));
    const bool hp = expert == CLOTHHIP_POLICY_HIGHEST_POINT;
    const size_t row = (size_t)3 * h->P, chunk = policy_eval_chunk(h->P), cmax = (size_t)n < chunk ? (size_t)n : chunk;
    if (obs_rows) if (int rc = h->pol.d_pe_rows.reserve(cmax * row * 4)) return rc;
    if (int rc = h->pol.d_pe_out.reserve(cmax * 4 * 8)) return rc;
    if (side) if (int rc = h->pol.d_pl_side.reserve(cmax * 4)) return rc;
    if (hp) if (int rc = h->pol.d_pl_choice.reserve(cmax * 4)) return rc;
    PolicyLabelArgs a;
    memset(&a, 0, sizeof(a));
    a.P = h->P; a.Ppad = h->Ppad; a.N = h->N; a.expert = expert; a.clip_act_space = clip_act_space; a.out = h->pol.d_pe_out;
    a.grid_dx = h->prm.width * 1.0 / (h->N - 1); a.grid_dy = h->prm.height * 1.0 / (h->N - 1);      // as fill_fused (api_run.hip)
    // the waves of a workgroup: as many rows' heights as 64 KB of LDS hold, four at the most (oracle corner stages nothing)
    const size_t zsize = obs_rows ? 4 : (h->precision == CLOTHHIP_F64 ? 8 : 4), zrow = (size_t)h->P * zsize;
    const int rpb = (int)std::min<size_t>(4, std::max<size_t>(1, ((size_t)64 << 10) / zrow));
    a.rows_per_block = rpb;
    const size_t lds = hp ? (size_t)rpb * zrow : 0;
    if (lds > ((size_t)64 << 10)) return fail(CLOTHHIP_ESTATE, "n_side %d: one row of heights needs %zu B of LDS (> 64 KiB)", h->N, lds);
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const size_t m = (size_t)n - i0 < chunk ? (size_t)n - i0 : chunk;
        a.n = (int64_t)m;
        if (side) { HIPCHECK(hipMemcpyAsync(h->pol.d_pl_side, side + i0, m * 4, hipMemcpyHostToDevice, h->stream)); a.side = h->pol.d_pl_side; }
        if (hp) { HIPCHECK(hipMemcpyAsync(h->pol.d_pl_choice, choice + i0, m * 4, hipMemcpyHostToDevice, h->stream)); a.choice = h->pol.d_pl_choice; }
        const dim3 grid((unsigned)((m + rpb - 1) / rpb)), block(64 * rpb);
        if (obs_rows) {
            HIPCHECK(hipMemcpyAsync(h->pol.d_pe_rows, obs_rows + i0 * row, m * row * 4, hipMemcpyHostToDevice, h->stream));
            a.rows = h->pol.d_pe_rows;
            HIPCHECK(hipEventRecord(h->ev0, h->stream));
            hipLaunchKernelGGL((k_policy_label<float, float>), grid, block, lds, h->stream, a);
        } else {
            HIPCHECK(hipEventRecord(h->ev0, h->stream));
            by_precision(h, [&](auto t) {
                using T = decltype(t);
                a.pos = (const T *)h->d_pos + i0 * 3 * h->Ppad;
                hipLaunchKernelGGL((k_policy_label<T, T>), grid, block, lds, h->stream, a);
            });
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(h->ev1, h->stream));
        h->have_timing = true;
        HIPCHECK(hipMemcpyAsync(actions_out + i0 * 4, h->pol.d_pe_out, m * 4 * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}
