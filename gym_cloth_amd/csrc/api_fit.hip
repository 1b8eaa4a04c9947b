// api_fit.hip -- the supervised trainer of the handle's networks, policy and critic, over the dataset of api_fit_data.hip: the loss and its gradient over a minibatch, the optimizer steps, advantages from the critic's values, the snapshot of the old means (and, with a log-sigma head, of the old log sigma; for a population by the member that acted) and PPO's clipped surrogate under a fixed or a learned sigma, of the shared network or of population rows under their own constants.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <utility>
#include <vector>

#include "api_handle.hpp"
#include "cloth_fit_ddpg.hpp"
#include "cloth_fit_gae.hpp"
#include "cloth_policy_fit.hpp"
#include "cloth_policy_mlp.hpp"

static_assert(FIT_MAX_BATCH == CLOTHHIP_FIT_MAX_BATCH, "the batch cap of the header and of the kernels");
static_assert(sizeof(ClothFitParams) == 24, "ClothFitParams is six floats");
static_assert(GAE_NEXT_NONE == CLOTHHIP_FIT_NEXT_NONE && CLOTHHIP_FIT_NEXT_TERMINAL < 0 && CLOTHHIP_FIT_NEXT_NONE < 0, "the leaf mark of the header and of the kernels");
static_assert(sizeof(ClothGaeParams) == 24, "ClothGaeParams is two doubles, a float and an int32");

// ---- the trainer (cloth_policy_fit.hpp has the definition and the order) ----------------------------------------------------------------
// ONE path: a call fits n_m rows of the handle's weight table in the launches of one network. The table is the population d_pop
// [pop_rows][mlp.stride], or the shared network d_mlp as a table of one row: the shared entries are the call members = {0}, n_m = 1 (row
// 0 lies at offset 0 whatever mlp.stride holds). The extern "C" entries below only refuse what each of them refuses and call it.
static_assert(CLOTHHIP_FIT_MAX_MEMBER_ROWS == 65536, "the header's cap on n_m * B of one call");

static const int32_t SHARED_ROW[1] = {0};      // the member list of the shared network, and of the value network

// The weight table a call trains, and what belongs to it: the policy's (shared network or population) or the value network's one row.
// The launches below read nothing else of the handle's networks.
struct FitNet {
    const MlpDesc &D;
    float *theta;                       // the table, [max(pop_rows, 1)][D.stride]
    size_t n_params;
    int64_t pop_rows;                   // 0: a table of one row at offset 0
    OptState &opt;                      // its optimizer
    bool value;                         // output width 1, fitted unweighted to the column of value targets; else width 4, to the labels under the weights
    int out() const { return value ? 1 : MLP_OUT; }
    size_t rows() const { return pop_rows ? (size_t)pop_rows : 1; }
};
static FitNet policy_net(clothhip_handle *h) {
    return {h->pol.mlp, h->pol.pop_rows ? h->pol.d_pop : h->pol.d_mlp, h->pol.mlp_n_params, h->pol.pop_rows, h->fit.opt_policy, false};
}
static FitNet value_net(clothhip_handle *h) { return {h->val.mlp, h->val.d_mlp, h->val.n_params, 0, h->fit.opt_value, true}; }

// What the entries refuse before anything is touched, each in the order it always had. The state; `population`: the entry trains rows of
// a population (which puts these refusals first, whatever else is wrong with the call), else the shared network
static int check_fit_state(const clothhip_handle *h, bool population) {
    if (int rc = check_idle(h)) return rc;
    if (population) {
        if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_population first");
        if (!h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds ONE shared network, not a population: use clothhip_policy_fit");
    } else {
        if (h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: the fit trains the ONE shared network of clothhip_set_policy_mlp");
        if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    }
    if (h->dataset.n < 1) return fail(CLOTHHIP_ESTATE, "the dataset is empty: call clothhip_fit_data_append first");
    return 0;
}
// ... and of the entries that train or evaluate the value network (a population is no obstacle: the critic is not the policy)
static int check_value_state(const clothhip_handle *h) {
    if (int rc = check_idle(h)) return rc;
    if (h->val.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no value network on this handle: call clothhip_set_value_mlp first");
    if (h->dataset.n < 1) return fail(CLOTHHIP_ESTATE, "the dataset is empty: call clothhip_fit_data_append first");
    return 0;
}
// the member list of a call ...
static int check_fit_members(const clothhip_handle *h, const int32_t *members, int32_t n_m) {
    if (n_m < 1) return fail(CLOTHHIP_EINVAL, "n_m = %d: a call names at least one member", n_m);
    if (!members) return fail(CLOTHHIP_EINVAL, "members is NULL");
    std::vector<uint8_t> seen;
    try { seen.assign((size_t)h->pol.pop_rows, 0); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)h->pol.pop_rows); }
    for (int32_t j = 0; j < n_m; j++) {
        if (members[j] < 0 || members[j] >= h->pol.pop_rows)
            return fail(CLOTHHIP_EINVAL, "members[%d] = %d outside [0, %lld)", j, members[j], (long long)h->pol.pop_rows);
        if (seen[members[j]]) return fail(CLOTHHIP_EINVAL, "members[%d] = %d is named twice: a call fits a row once", j, members[j]);
        seen[members[j]] = 1;
    }
    return 0;
}
// ... its minibatches: n_idx entries of idx in all, B rows per member and step ...
static int check_fit_rows(const clothhip_handle *h, int32_t n_m, const int32_t *idx, int64_t n_idx, int32_t B) {
    if (B < 1 || B > FIT_MAX_BATCH) return fail(CLOTHHIP_EINVAL, "B = %d outside [1, %d]", B, FIT_MAX_BATCH);
    if ((int64_t)n_m * B > CLOTHHIP_FIT_MAX_MEMBER_ROWS)
        return fail(CLOTHHIP_EINVAL, "n_m * B = %d * %d rows in one call, at most %d", n_m, B, CLOTHHIP_FIT_MAX_MEMBER_ROWS);
    if (!idx && n_idx > 0) return fail(CLOTHHIP_EINVAL, "idx is NULL");
    for (int64_t i = 0; i < n_idx; i++)
        if (idx[i] < 0 || idx[i] >= h->dataset.n) return fail(CLOTHHIP_EINVAL, "idx[%lld] = %d outside [0, %lld)", (long long)i, idx[i], (long long)h->dataset.n);
    return 0;
}
// ... and the optimizer of member j (j < 0: the one of the shared network, named without an index)
static bool hyper_ok(float v) { return std::isfinite(v) && v >= 0.0f; }
static int check_fit_params(const ClothFitParams *p, int32_t j) {
    char who[24] = "";
    if (j >= 0) snprintf(who, sizeof(who), "p[%d]: ", j);
    if (p->optimizer != (float)CLOTHHIP_FIT_ADAM && p->optimizer != (float)CLOTHHIP_FIT_SGD)
        return fail(CLOTHHIP_EINVAL, "%sunknown optimizer %g (CLOTHHIP_FIT_ADAM or CLOTHHIP_FIT_SGD)", who, (double)p->optimizer);
    if (!hyper_ok(p->lr) || !hyper_ok(p->eps) || !hyper_ok(p->momentum) || !hyper_ok(p->beta1) || !hyper_ok(p->beta2))
        return fail(CLOTHHIP_EINVAL, "%sa hyper-parameter is negative or not finite (lr %g, beta1 %g, beta2 %g, eps %g, momentum %g)", who, (double)p->lr,
                    (double)p->beta1, (double)p->beta2, (double)p->eps, (double)p->momentum);
    if (p->beta1 >= 1.0f || p->beta2 >= 1.0f) return fail(CLOTHHIP_EINVAL, "%sbeta1 %g, beta2 %g: both lie in [0, 1)", who, (double)p->beta1, (double)p->beta2);
    return 0;
}

// ... and the optimizers p [n_m] of a grouped step entry: each valid by its index, and one optimizer per call
static int check_fit_params_members(const ClothFitParams *p, int32_t n_m) {
    for (int32_t j = 0; j < n_m; j++) {
        if (int rc = check_fit_params(p + j, j)) return rc;
        if (p[j].optimizer != p[0].optimizer) return fail(CLOTHHIP_EINVAL, "p[%d].optimizer = %g, p[0].optimizer = %g: one optimizer per call", j, (double)p[j].optimizer, (double)p[0].optimizer);
    }
    return 0;
}

// Where member j's tables lie: the per-member sizes of the scratch tables (floats) for minibatches of B rows, and the offsets of every
// layer inside a blob (weights, gradient) and inside a member's activations.
struct FitPlan {
    size_t act, dz, part, grad, maxw;       // per member: activations, the two dZ tables, the slabs (0 without a split), the gradient
    int n_split;
    size_t w_off[MLP_MAX_LAYERS], h_off[MLP_MAX_LAYERS];
};
static FitPlan fit_plan(const FitNet &net, int32_t B) {
    const MlpDesc &D = net.D;
    FitPlan p = {};
    size_t maxmat = 0;
    p.maxw = MLP_OUT;
    for (int l = 0; l < D.n_layers; l++) {
        p.w_off[l] = p.grad; p.h_off[l] = p.act;
        p.grad += (size_t)D.widths[l + 1] * D.widths[l] + D.widths[l + 1];
        p.act += (size_t)B * D.widths[l + 1];
        p.maxw = std::max<size_t>(p.maxw, D.widths[l + 1]);
        maxmat = std::max<size_t>(maxmat, (size_t)D.widths[l + 1] * D.widths[l]);
    }
    p.dz = 2 * (size_t)B * p.maxw;
    p.n_split = (B + FIT_SPLIT_ROWS - 1) / FIT_SPLIT_ROWS;
    p.part = p.n_split > 1 ? (size_t)p.n_split * maxmat : 0;
    return p;
}
// one step's scratch for n_m members
static int fit_reserve(clothhip_handle *h, const FitPlan &p, int32_t n_m) {
    auto &f = h->fit;
    if (int rc = f.d_members.reserve((size_t)n_m * 4)) return rc;
    if (int rc = f.d_act.reserve((size_t)n_m * p.act * 4)) return rc;
    if (int rc = f.d_dz.reserve((size_t)n_m * p.dz * 4)) return rc;
    if (p.part) if (int rc = f.d_part.reserve((size_t)n_m * p.part * 4)) return rc;
    return f.d_grad.reserve((size_t)n_m * p.grad * 4);
}

// The tables a pass of one network works on: its activations, the two dZ tables, the slabs of a split batch sum, the gradient (each
// NULL where the pass does not touch it), and its layer-0 input -- x NULL: the dataset's observation rows through the call's index
// table, else dense rows [B][widths[0]] (the critic's [s, a] rows of DDPG). The trainer's own scratch is policy_work(h), valid after fit_reserve.
struct FitWork { float *act, *dz, *part, *grad; const float *x; };
static FitWork policy_work(clothhip_handle *h) { return {h->fit.d_act, h->fit.d_dz, h->fit.d_part, h->fit.d_grad, nullptr}; }

template <bool A_KC, bool B_KC, int EPI, bool ROWS> static void launch_gemm(hipStream_t s, FitGemmArgs &a, int32_t n_m) {
    a.tiles_n = (a.N + FIT_TILE - 1) / FIT_TILE;
    const dim3 grid((unsigned)a.tiles_n * (unsigned)n_m, (unsigned)((a.M + FIT_TILE - 1) / FIT_TILE), (unsigned)((a.K + a.k_chunk - 1) / a.k_chunk));
    hipLaunchKernelGGL((k_fit_gemm<A_KC, B_KC, EPI, ROWS>), grid, dim3(FIT_THREADS), 0, s, a);
}

// What a step minimises, with the fields that loss reads and no others. The width of the squared error comes from FitNet; both
// surrogates are the policy's table only. A new loss is one more kind, its fields, and its case in enqueue_loss.
struct FitLoss {
    enum Kind { SQUARED_ERROR, PPO, PPO_SIGMA } kind;
    int stats;                                      // doubles per member and step in the loss table: the loss, or the surrogate's statistics
    union {
        const double *q;                            // PPO: host [n_m][4] {inv_s2, half_inv_s2, lo, hi}, row j member j's (check_ppo makes it)
        struct { double lo, hi, ent_coef; } s;      // PPO_SIGMA: 1 - eps, 1 + eps and the entropy coefficient; 1 / sigma^2 comes from the head
    };
};
static FitLoss squared_error() { FitLoss l = {}; l.kind = FitLoss::SQUARED_ERROR; l.stats = 1; return l; }
static FitLoss ppo_loss(const double *q) { FitLoss l = {}; l.kind = FitLoss::PPO; l.stats = FIT_PPO_STATS; l.q = q; return l; }
static FitLoss ppo_sigma_loss(double lo, double hi, double ent_coef) { FitLoss l = {}; l.kind = FitLoss::PPO_SIGMA; l.stats = FIT_PPO_SIGMA_STATS; l.s = {lo, hi, ent_coef}; return l; }

// Where a call's results go on the host, each NULL when the caller does not want it: loss [n_steps][n_m][stats]; of a gradient call grad
// [n_m][n_params], ratio [n_m][B] (the surrogates), grad_ls [4] (PPO_SIGMA); of a PPO_SIGMA fit ls [n_steps][4], the head before each update
struct FitOut { double *loss; float *grad, *ratio, *grad_ls, *ls; };

// The launches of one network's step, each over all n_m members: forward, loss, backward. The forward of the present weights over rows
// d_idx [n_m][B]: member j's y is then at h->fit.d_act + j * p.act + p.h_off[L - 1].
// shared_rows: d_idx is ONE list [B] that every member reads
static int enqueue_forward(clothhip_handle *h, const FitNet &net, const FitPlan &p, int32_t n_m, const int32_t *d_idx, int32_t B, bool shared_rows,
                           const FitWork &w) {
    const MlpDesc &D = net.D;
    const int L = D.n_layers;
    float *act = w.act;
    FitGemmArgs m0 = {};
    m0.members = h->fit.d_members; m0.stride = D.stride; m0.rows_step = shared_rows ? 0 : B;
    for (int l = 0; l < L; l++) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        FitGemmArgs a = m0;
        const bool gather = l == 0 && !w.x;      // layer 0 reads the dataset through the index table, unless the pass has its own input rows
        a.A = l ? act + p.h_off[l - 1] : gather ? (const float *)h->dataset.obs() : w.x; a.lda = n_in; a.rows = gather ? d_idx : nullptr; a.a_step = l ? (int64_t)p.act : 0;
        a.B = D.params + p.w_off[l]; a.ldb = n_in; a.bias = a.B + (size_t)n_out * n_in; a.b_weights = 1;
        a.C = act + p.h_off[l]; a.ldc = n_out; a.c_step = (int64_t)p.act;
        a.M = B; a.N = n_out; a.K = n_in; a.k_chunk = n_in;
        if (gather && l + 1 < L) launch_gemm<true, true, FIT_EPI_BIAS_RELU, true>(h->stream, a, n_m);
        else if (gather) launch_gemm<true, true, FIT_EPI_BIAS, true>(h->stream, a, n_m);
        else if (l + 1 < L) launch_gemm<true, true, FIT_EPI_BIAS_RELU, false>(h->stream, a, n_m);
        else launch_gemm<true, true, FIT_EPI_BIAS, false>(h->stream, a, n_m);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}
// The loss of the forward's y and its dZ of the last layer: d_stats [n_m][loss.stats]. The surrogates: d_ratio (may be NULL) [n_m][B];
// PPO reads member j's constants from row j of h->fit.d_ppo_q (the caller has uploaded loss.q); PPO_SIGMA reads the handle's log-sigma
// head where it lies, writes the head's gradient to h->fit.d_grad_ls and the head it read to d_ls (may be NULL)
static int enqueue_loss(clothhip_handle *h, const FitNet &net, const FitPlan &p, const FitLoss &loss, int32_t n_m, const int32_t *d_idx, int32_t B, double *d_stats,
                        float *d_ratio, float *d_ls) {
    auto &f = h->fit;
    const auto &d = h->dataset;
    const int L = net.D.n_layers;
    const float *y = f.d_act + p.h_off[L - 1];
    float *dz = f.d_dz + ((L - 1) & 1) * (size_t)B * p.maxw;
    const dim3 grid((unsigned)n_m), block(256);
    if (loss.kind == FitLoss::PPO_SIGMA) {
        FitPpoSigmaArgs q = {};
        q.y = y; q.lab = d.lab(); q.old = d.old(); q.old_ls = d.old_ls(); q.wgt = d.w(); q.ls = h->pol.d_log_sigma; q.rows = d_idx;
        q.dz = dz; q.ratio = d_ratio; q.grad_ls = f.d_grad_ls; q.ls_out = d_ls; q.stats = d_stats;
        q.lo = loss.s.lo; q.hi = loss.s.hi; q.ent_coef = loss.s.ent_coef;
        q.y_step = (int64_t)p.act; q.dz_step = (int64_t)p.dz; q.rows_step = (int64_t)B; q.B = B;
        hipLaunchKernelGGL(k_fit_loss_ppo_sigma, grid, block, 0, h->stream, q);
    } else if (loss.kind == FitLoss::PPO) {
        FitPpoArgs q = {};
        q.y = y; q.lab = d.lab(); q.old = d.old(); q.wgt = d.w(); q.rows = d_idx; q.dz = dz; q.ratio = d_ratio; q.stats = d_stats; q.q = f.d_ppo_q;
        q.y_step = (int64_t)p.act; q.dz_step = (int64_t)p.dz; q.rows_step = (int64_t)B; q.B = B;
        hipLaunchKernelGGL(k_fit_loss_ppo, grid, block, 0, h->stream, q);
    } else if (net.value)      // SQUARED_ERROR, at the net's width
        hipLaunchKernelGGL(k_fit_loss<1>, grid, block, 0, h->stream, y, (const float *)d.ret(), (const float *)nullptr, d_idx, B, dz, d_stats, (int64_t)p.act, (int64_t)p.dz, (int64_t)B);
    else
        hipLaunchKernelGGL(k_fit_loss<4>, grid, block, 0, h->stream, y, (const float *)d.lab(), (const float *)d.w(), d_idx, B, dz, d_stats, (int64_t)p.act, (int64_t)p.dz, (int64_t)B);
    HIPCHECK(hipGetLastError());
    return 0;
}
// The backward from the loss launch's dZ: the gradient of every member into h->fit.d_grad [n_m][n_params] (blob layout)
static int enqueue_backward(clothhip_handle *h, const FitNet &net, const FitPlan &p, int32_t n_m, const int32_t *d_idx, int32_t B, const FitWork &w) {
    const MlpDesc &D = net.D;
    auto &f = h->fit;
    float *act = w.act, *grad = w.grad, *dz[2] = {w.dz, w.dz + (size_t)B * p.maxw};
    FitGemmArgs m0 = {};
    m0.members = f.d_members; m0.stride = D.stride; m0.rows_step = B;
    for (int l = D.n_layers - 1; l >= 0; l--) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        const float *dzl = dz[l & 1];
        float *gWl = grad + p.w_off[l];
        FitGemmArgs a = m0;
        a.A = dzl; a.lda = n_out; a.a_step = (int64_t)p.dz;
        const bool gather = l == 0 && !w.x;
        a.B = l ? act + p.h_off[l - 1] : gather ? (const float *)h->dataset.obs() : w.x; a.ldb = n_in; a.rows = gather ? d_idx : nullptr; a.b_step = l ? (int64_t)p.act : 0;
        a.C = p.n_split > 1 ? w.part : gWl; a.ldc = n_in; a.c_slab = (int64_t)n_out * n_in; a.c_step = (int64_t)(p.n_split > 1 ? p.part : p.grad);
        a.M = n_out; a.N = n_in; a.K = B; a.k_chunk = FIT_SPLIT_ROWS;
        if (gather) launch_gemm<false, false, FIT_EPI_NONE, true>(h->stream, a, n_m);
        else launch_gemm<false, false, FIT_EPI_NONE, false>(h->stream, a, n_m);
        HIPCHECK(hipGetLastError());
        if (p.n_split > 1) {
            const int64_t n = (int64_t)n_out * n_in;
            const int32_t blocks = (int32_t)((n + 255) / 256);
            hipLaunchKernelGGL(k_fit_reduce, dim3((unsigned)blocks * (unsigned)n_m), dim3(256), 0, h->stream, (const float *)w.part, n, p.n_split, gWl, n,
                               (int64_t)p.part, (int64_t)p.grad, blocks);
            HIPCHECK(hipGetLastError());
        }
        const int32_t cblocks = (n_out + 63) / 64;
        hipLaunchKernelGGL(k_fit_colsum, dim3((unsigned)cblocks * (unsigned)n_m), dim3(64), 0, h->stream, dzl, B, n_out, gWl + (size_t)n_out * n_in,
                           (int64_t)p.dz, (int64_t)p.grad, cblocks);
        HIPCHECK(hipGetLastError());
        if (l > 0) {
            FitGemmArgs b = m0;
            b.A = dzl; b.lda = n_out; b.a_step = (int64_t)p.dz;
            b.B = D.params + p.w_off[l]; b.ldb = n_in; b.b_weights = 1;
            b.mask = act + p.h_off[l - 1]; b.mask_step = (int64_t)p.act;
            b.C = dz[(l - 1) & 1]; b.ldc = n_in; b.c_step = (int64_t)p.dz;
            b.M = B; b.N = n_in; b.K = n_out; b.k_chunk = n_out;
            launch_gemm<true, false, FIT_EPI_MASK, false>(h->stream, b, n_m);
            HIPCHECK(hipGetLastError());
        }
    }
    return 0;
}
// ... and all three: loss and gradient of the present weights over rows d_idx [n_m][B], every member on its own rows
static int enqueue_grad(clothhip_handle *h, const FitNet &net, const FitPlan &p, const FitLoss &loss, int32_t n_m, const int32_t *d_idx, int32_t B, double *d_stats,
                        float *d_ratio, float *d_ls) {
    if (int rc = enqueue_forward(h, net, p, n_m, d_idx, B, false, policy_work(h))) return rc;
    if (int rc = enqueue_loss(h, net, p, loss, n_m, d_idx, B, d_stats, d_ratio, d_ls)) return rc;
    return enqueue_backward(h, net, p, n_m, d_idx, B, policy_work(h));
}

// loss and gradient of `members` over idx [n_m][B], nothing updated; the call is valid
static int run_grad(clothhip_handle *h, const FitNet &net, const FitLoss &loss, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B, const FitOut &out) {
    auto &f = h->fit;
    const FitPlan p = fit_plan(net, B);
    const size_t n_loss = (size_t)n_m * loss.stats;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, p, n_m)) return rc;
    if (loss.kind == FitLoss::PPO_SIGMA) if (int rc = f.d_grad_ls.reserve((size_t)n_m * MLP_OUT * 4)) return rc;
    if (int rc = f.d_idx.reserve((size_t)n_m * B * 4)) return rc;
    if (int rc = f.d_loss.reserve(n_loss * 8)) return rc;
    if (out.ratio) if (int rc = f.d_ratio.reserve((size_t)n_m * B * 4)) return rc;
    if (loss.kind == FitLoss::PPO) {      // the members' constants, one row for the shared network
        if (int rc = f.d_ppo_q.reserve((size_t)n_m * 32)) return rc;
        HIPCHECK(hipMemcpyAsync(f.d_ppo_q, loss.q, (size_t)n_m * 32, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHECK(hipMemcpyAsync(f.d_members, members, (size_t)n_m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)n_m * B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    if (int rc = enqueue_grad(h, net, p, loss, n_m, f.d_idx, B, f.d_loss, out.ratio ? (float *)f.d_ratio : nullptr, nullptr)) return rc;
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    if (out.grad) HIPCHECK(hipMemcpyAsync(out.grad, f.d_grad, (size_t)n_m * p.grad * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.loss) HIPCHECK(hipMemcpyAsync(out.loss, f.d_loss, n_loss * 8, hipMemcpyDeviceToHost, h->stream));
    if (out.ratio) HIPCHECK(hipMemcpyAsync(out.ratio, f.d_ratio, (size_t)n_m * B * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.grad_ls) HIPCHECK(hipMemcpyAsync(out.grad_ls, f.d_grad_ls, (size_t)n_m * MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_fit_grad(clothhip_handle *h, const int32_t *idx, int32_t B, float *grad_out, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    return run_grad(h, policy_net(h), squared_error(), SHARED_ROW, 1, idx, B, {loss_out, grad_out});
}

extern "C" int clothhip_policy_fit_grad_members(clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B, float *grad_out,
                                                double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_m * B, B)) return rc;
    return run_grad(h, policy_net(h), squared_error(), members, n_m, idx, B, {loss_out, grad_out});
}

// The loss alone of the shared network over any number of rows: chunks of at most FIT_MAX_BATCH through the forward pass above, each
// chunk's weighted sum of squares in k_fit_loss's order (k_fit_sqsum), the chunk sums added in ascending order in double on the host, divided
// once by 4 n.
extern "C" int clothhip_policy_fit_loss(clothhip_handle *h, const int32_t *idx, int64_t n, double *loss) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    const int32_t Bmax = (int32_t)std::min<int64_t>(n, FIT_MAX_BATCH);
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, n, Bmax)) return rc;
    if (!loss) return fail(CLOTHHIP_EINVAL, "NULL argument");
    auto &f = h->fit;
    const FitNet net = policy_net(h);
    const int L = h->pol.mlp.n_layers;
    const int64_t n_chunks = (n + FIT_MAX_BATCH - 1) / FIT_MAX_BATCH;
    std::vector<double> sums;
    try { sums.resize((size_t)n_chunks); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld chunks)", (long long)n_chunks); }
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, fit_plan(net, Bmax), 1)) return rc;
    if (int rc = f.d_idx.reserve((size_t)n * 4)) return rc;
    if (int rc = f.d_loss.reserve((size_t)n_chunks * 8)) return rc;
    HIPCHECK(hipMemcpyAsync(f.d_members, SHARED_ROW, 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int64_t c = 0; c < n_chunks; c++) {
        const int32_t B = (int32_t)std::min<int64_t>(FIT_MAX_BATCH, n - c * FIT_MAX_BATCH);
        const FitPlan p = fit_plan(net, B);
        const int32_t *d_idx = f.d_idx + (size_t)c * FIT_MAX_BATCH;
        if (int rc = enqueue_forward(h, net, p, 1, d_idx, B, false, policy_work(h))) return rc;
        launch_fit_sqsum(h->stream, f.d_act + p.h_off[L - 1], h->dataset.lab(), h->dataset.w(), d_idx, B, f.d_loss + c);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipMemcpyAsync(sums.data(), f.d_loss, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    double s = sums[0];
    for (int64_t c = 1; c < n_chunks; c++) s = s + sums[c];
    *loss = s / (double)(4 * n);
    return 0;
}

// The forward alone on n stored rows, the same rows for every member: chunks through enqueue_forward, each chunk's y copied out to
// d_pred [n_m][n][net.out()] (k_fit_copy_y), where it stays: enqueued between the timing events, not synchronised. The call is valid.
// dst (NULL: d_pred; else n_m == 1): the table that gets y in the place of d_pred, [n][net.out()] -- a dataset column that is written where it lies.
static int enqueue_predict(clothhip_handle *h, const FitNet &net, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *dst) {
    auto &f = h->fit;
    const int L = net.D.n_layers, W = net.out();
    const int32_t Bmax = (int32_t)std::min<int64_t>(n, std::min<int64_t>(FIT_MAX_BATCH, CLOTHHIP_FIT_MAX_MEMBER_ROWS / n_m));
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, fit_plan(net, Bmax), n_m)) return rc;
    if (int rc = f.d_idx.reserve((size_t)n * 4)) return rc;
    if (!dst) {
        if (int rc = f.d_pred.reserve((size_t)n_m * n * W * 4)) return rc;
        dst = f.d_pred;
    }
    HIPCHECK(hipMemcpyAsync(f.d_members, members, (size_t)n_m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int64_t r0 = 0; r0 < n; r0 += Bmax) {
        const int32_t B = (int32_t)std::min<int64_t>(Bmax, n - r0);
        const FitPlan p = fit_plan(net, B);
        if (int rc = enqueue_forward(h, net, p, n_m, f.d_idx + (size_t)r0, B, true, policy_work(h))) return rc;
        const int32_t blocks = (W * B + 255) / 256;
        launch_fit_copy_y(h->stream, n_m, f.d_act + p.h_off[L - 1], W * B, dst + (size_t)r0 * W, (int64_t)p.act, (int64_t)n * W, blocks);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    return 0;
}
// ... and one download
static int run_predict(clothhip_handle *h, const FitNet &net, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *y_out) {
    if (int rc = enqueue_predict(h, net, members, n_m, idx, n, nullptr)) return rc;
    HIPCHECK(hipMemcpyAsync(y_out, h->fit.d_pred, (size_t)n_m * n * net.out() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_fit_predict(clothhip_handle *h, const int32_t *idx, int64_t n, float *y_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, n, (int32_t)std::min<int64_t>(n, FIT_MAX_BATCH))) return rc;
    if (!y_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    return run_predict(h, policy_net(h), SHARED_ROW, 1, idx, n, y_out);
}

extern "C" int clothhip_policy_fit_predict_members(clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *y_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (n_m > CLOTHHIP_FIT_MAX_MEMBER_ROWS) return fail(CLOTHHIP_EINVAL, "n_m = %d members in one call, at most %d", n_m, CLOTHHIP_FIT_MAX_MEMBER_ROWS);
    if (int rc = check_fit_rows(h, 1, idx, n, 1)) return rc;
    if (!y_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    return run_predict(h, policy_net(h), members, n_m, idx, n, y_out);
}

// ---- the optimizer ----------------------------------------------------------------------------------------------------------------------
// the per-row optimizer state exists from the first step after a new network: every row fresh. false: out of host memory, and forgotten
static bool ensure_row_state(OptState &o, size_t rows) {
    if (o.t.size() == rows && o.zero.size() == rows) return true;
    try { o.t.assign(rows, 0); o.zero.assign(rows, 1); } catch (const std::bad_alloc &) { o.forget(); return false; }
    return true;
}

// The step constants q [FIT_HYPER] of ONE optimizer step under p, the t1-th of its row (1-based): made in double, then rounded to float
static void step_constants(float *q, const ClothFitParams &p, bool adam, int64_t t1) {
    if (adam) {
        const double b1 = (double)p.beta1, b2 = (double)p.beta2, td = (double)t1;
        const double a_t = (double)p.lr * std::sqrt(1.0 - std::pow(b2, td)) / (1.0 - std::pow(b1, td));
        q[0] = (float)a_t; q[1] = p.beta1; q[2] = (float)(1.0 - b1); q[3] = p.beta2; q[4] = (float)(1.0 - b2); q[5] = p.eps;
    } else {
        q[0] = p.lr; q[1] = p.momentum;
    }
}
// One optimizer launch: the rows h->fit.d_members [n_m] of theta ([rows][stride], n elements each) with the moments of opt, row j's
// gradient at grad + j * n and its constants at d_hyper + j * FIT_HYPER (device)
static int enqueue_optimizer(clothhip_handle *h, bool adam, float *theta, OptState &opt, const float *grad, const float *d_hyper, int64_t stride, int64_t n, int32_t n_m) {
    FitOptArgs o = {};
    o.theta = theta; o.m = opt.m; o.v = opt.v; o.g = grad; o.members = h->fit.d_members;
    o.hyper = d_hyper;
    o.stride = stride; o.n = n; o.blocks = (int32_t)((n + 255) / 256);
    const dim3 ogrid((unsigned)o.blocks * (unsigned)n_m);
    if (adam) hipLaunchKernelGGL(k_fit_adam, ogrid, dim3(256), 0, h->stream, o);
    else hipLaunchKernelGGL(k_fit_sgd, ogrid, dim3(256), 0, h->stream, o);
    HIPCHECK(hipGetLastError());
    return 0;
}

// One table the optimizer updates in a step of a call: the rows `members` [n_m] of theta, n elements each at members[j] * stride, with
// the moments and step counts of `opt`; row j's gradient lies at grad + j * n, and its step constants are made from p[j].
struct FitTarget {
    float *theta;
    OptState &opt;
    size_t moments;                     // floats of each moment table
    int64_t stride, n;
    const int32_t *members;             // host
    int32_t n_m;
    const Buffer<float> &grad;          // (a pointer only after the call's reserves)
    const ClothFitParams *p;
};

// n_steps optimizer steps of `members` with the optimizers p [n_m] over idx [n_steps][n_m][B]; the call is valid and n_steps >= 1. The
// optimizer walks one target, the net's rows, and under PPO_SIGMA (n_m == 1) a second one: the log-sigma head, a table of one row of
// four elements at offset 0 with its own state h->fit.opt_sigma and its own step constants, made from p[0]. Target k's step constants
// follow those of the targets before it in ONE table, [n_steps][its n_m][FIT_HYPER] each
static int run_fit(clothhip_handle *h, const FitNet &net, const FitLoss &loss, const ClothFitParams *p, const int32_t *members, int32_t n_m, const int32_t *idx,
                   int32_t n_steps, int32_t B, const FitOut &out) {
    const bool adam = p[0].optimizer == (float)CLOTHHIP_FIT_ADAM;
    auto &f = h->fit;
    const FitPlan pl = fit_plan(net, B);
    const size_t n_sm = (size_t)n_steps * n_m;
    const bool head = loss.kind == FitLoss::PPO_SIGMA;
    const FitTarget targets[2] = {
        {net.theta, net.opt, net.pop_rows ? (size_t)net.pop_rows * net.D.stride : net.n_params, (int64_t)net.D.stride, (int64_t)net.n_params, members, n_m, f.d_grad, p},
        {h->pol.d_log_sigma, f.opt_sigma, MLP_OUT, 0, MLP_OUT, SHARED_ROW, 1, f.d_grad_ls, p}};
    const int n_targets = head ? 2 : 1;
    // the step constants of every (target, step, member), in double on the host, then rounded to float; nothing of the handle changes yet
    size_t hyper_at[2], n_hyper = 0;
    for (int k = 0; k < n_targets; k++) { hyper_at[k] = n_hyper; n_hyper += (size_t)n_steps * targets[k].n_m * FIT_HYPER; }
    std::vector<float> hyper;
    try { hyper.assign(n_hyper, 0.0f); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%zu step constants)", n_hyper); }
    if (!ensure_row_state(net.opt, net.rows())) return fail(CLOTHHIP_ENOMEM, "out of host memory (%zu rows)", net.rows());
    if (head && !ensure_row_state(f.opt_sigma, 1)) return fail(CLOTHHIP_ENOMEM, "out of host memory (the head's optimizer state)");
    for (int k = 0; k < n_targets; k++) {
        const FitTarget &t = targets[k];
        for (int s = 0; s < n_steps; s++)
            for (int32_t j = 0; j < t.n_m; j++) {
                step_constants(hyper.data() + hyper_at[k] + ((size_t)s * t.n_m + j) * FIT_HYPER, t.p[j], adam, t.opt.t[t.members[j]] + s + 1);
            }
    }
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, pl, n_m)) return rc;
    if (int rc = f.d_idx.reserve(n_sm * B * 4)) return rc;
    if (int rc = f.d_loss.reserve(n_sm * loss.stats * 8)) return rc;
    if (int rc = f.d_hyper.reserve(n_hyper * 4)) return rc;
    if (loss.kind == FitLoss::PPO) if (int rc = f.d_ppo_q.reserve((size_t)n_m * 32)) return rc;
    if (head) {
        if (int rc = f.d_grad_ls.reserve(MLP_OUT * 4)) return rc;
        if (int rc = f.d_ls_hist.reserve((size_t)n_steps * MLP_OUT * 4)) return rc;
    }
    // the moments of each target's whole table. A table of another network's size holds no row's state (every row is flagged
    // read-as-zeros by OptState::forget when the network changes), so growing it loses nothing
    for (int k = 0; k < n_targets; k++) {
        if (int rc = targets[k].opt.m.reserve(targets[k].moments * 4)) return rc;
        if (int rc = targets[k].opt.v.reserve(targets[k].moments * 4)) return rc;
    }
    // from here on the call goes through (but for a failure of the runtime itself)
    for (int k = 0; k < n_targets; k++) {
        const FitTarget &t = targets[k];
        for (int32_t j = 0; j < t.n_m; j++) {
            const int32_t g = t.members[j];
            if (t.opt.zero[g]) {
                HIPCHECK(hipMemsetAsync(t.opt.m + (size_t)g * (size_t)t.stride, 0, (size_t)t.n * 4, h->stream));
                HIPCHECK(hipMemsetAsync(t.opt.v + (size_t)g * (size_t)t.stride, 0, (size_t)t.n * 4, h->stream));
                t.opt.zero[g] = 0;
            }
            t.opt.t[g] += n_steps;
        }
    }
    HIPCHECK(hipMemcpyAsync(f.d_members, members, (size_t)n_m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, n_sm * B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_hyper, hyper.data(), n_hyper * 4, hipMemcpyHostToDevice, h->stream));
    if (loss.kind == FitLoss::PPO) HIPCHECK(hipMemcpyAsync(f.d_ppo_q, loss.q, (size_t)n_m * 32, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int s = 0; s < n_steps; s++) {
        if (int rc = enqueue_grad(h, net, pl, loss, n_m, f.d_idx + (size_t)s * n_m * B, B, f.d_loss + (size_t)s * n_m * loss.stats, nullptr,
                                  head ? f.d_ls_hist + (size_t)s * MLP_OUT : nullptr)) return rc;
        for (int k = 0; k < n_targets; k++) {      // (the head names its row 0 by the call's own member table: n_m == 1, members = {0})
            const FitTarget &t = targets[k];
            if (int rc = enqueue_optimizer(h, adam, t.theta, t.opt, t.grad, f.d_hyper + hyper_at[k] + (size_t)s * t.n_m * FIT_HYPER, t.stride, t.n, t.n_m)) return rc;
        }
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    if (out.loss) HIPCHECK(hipMemcpyAsync(out.loss, f.d_loss, n_sm * loss.stats * 8, hipMemcpyDeviceToHost, h->stream));
    if (head && out.ls) HIPCHECK(hipMemcpyAsync(out.ls, f.d_ls_hist, (size_t)n_steps * MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // (the host tables are never retained)
    return 0;
}

extern "C" int clothhip_policy_fit(clothhip_handle *h, const ClothFitParams *p, const int32_t *idx, int32_t n_steps, int32_t B, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), squared_error(), p, SHARED_ROW, 1, idx, n_steps, B, {loss_out});
}

extern "C" int clothhip_policy_fit_members(clothhip_handle *h, const ClothFitParams *p, const int32_t *members, int32_t n_m, const int32_t *idx,
                                           int32_t n_steps, int32_t B, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_steps * n_m * B, B)) return rc;
    if (int rc = check_fit_params_members(p, n_m)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), squared_error(), p, members, n_m, idx, n_steps, B, {loss_out});
}

extern "C" int clothhip_policy_fit_reset(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit.opt_policy.forget();
    h->fit.opt_sigma.forget();      // the head is trained with the policy
    return 0;
}

extern "C" int clothhip_policy_fit_reset_members(clothhip_handle *h, const int32_t *members, int32_t n_m) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_population first");
    if (!h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds ONE shared network, not a population: use clothhip_policy_fit_reset");
    if (!members) { h->fit.opt_policy.forget(); return 0; }      // all rows
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (h->fit.opt_policy.t.empty()) return 0;               // every row is fresh already
    for (int32_t j = 0; j < n_m; j++) { h->fit.opt_policy.t[members[j]] = 0; h->fit.opt_policy.zero[members[j]] = 1; }
    return 0;
}

// ---- PPO: the old means and the clipped surrogate as one more loss mode of the trainer above (clothhip.h: PPO ON THE DEVICE) --------------
static_assert(FIT_PPO_STATS == CLOTHHIP_PPO_STATS, "the statistics of the header and of the kernel");
static_assert(sizeof(ClothPpoParams) == 16, "ClothPpoParams is two doubles");

extern "C" int clothhip_fit_data_snapshot_policy(clothhip_handle *h, int64_t first, int64_t n) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_range(h, first, n)) return rc;
    if (n == 0) return 0;
    std::vector<int32_t> idx;
    try { idx.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); }
    for (int64_t i = 0; i < n; i++) idx[(size_t)i] = (int32_t)(first + i);
    // the launches of clothhip_policy_fit_predict; each chunk's y goes to its rows of the column, which are consecutive
    if (int rc = enqueue_predict(h, policy_net(h), SHARED_ROW, 1, idx.data(), n, h->dataset.old() + (size_t)first * 4)) return rc;
    // with a head: the present log sigma into the same rows of its column, on the device (the predict moved ev1 behind itself; so does this)
    if (h->pol.has_log_sigma) {
        const int64_t n4 = n * MLP_OUT;
        hipLaunchKernelGGL(k_fit_fill_ls, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, h->stream, h->dataset.old_ls() + (size_t)first * MLP_OUT, (const float *)h->pol.d_log_sigma, n4);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(h->ev1, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));      // (idx, a host table the upload read, goes out of scope)
    h->dataset.mark_old_set(first, n);
    if (h->pol.has_log_sigma) h->dataset.mark_old_ls_set(first, n);
    return 0;
}

// the constants of member j of a PPO call (j < 0: of the shared network, named without an index) -> row [4], the kernel's constants
static int check_ppo_consts(const ClothPpoParams *q, int32_t j, double *row) {
    char who[24] = "";
    if (j >= 0) snprintf(who, sizeof(who), "q[%d]: ", j);
    if (!std::isfinite(q->sigma) || q->sigma <= 0.0) return fail(CLOTHHIP_EINVAL, "%ssigma = %g: the policy's standard deviation is finite and > 0", who, q->sigma);
    if (!std::isfinite(q->clip) || q->clip < 0.0 || q->clip >= 1.0) return fail(CLOTHHIP_EINVAL, "%sclip = %g: the clip range lies in [0, 1)", who, q->clip);
    const double s2 = q->sigma * q->sigma;
    row[0] = 1.0 / s2;
    row[1] = 0.5 * row[0];
    row[2] = 1.0 - q->clip;
    row[3] = 1.0 + q->clip;
    if (!std::isfinite(row[0])) return fail(CLOTHHIP_EINVAL, "%ssigma = %g: 1 / sigma^2 is not a finite double", who, q->sigma);
    return 0;
}
// every row of the minibatches idx [n_steps][n_m][B] (n_idx entries) has its old mean and, log_sigma: its old log sigma. members
// NULL: the shared network's call (n_m == 1), else the refusal names the member whose row it is
static int check_old_set(const clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n_idx, int32_t B, bool log_sigma) {
    for (int64_t i = 0; i < n_idx; i++) {
        if (!h->dataset.h_old_set[(size_t)idx[i]]) {
            char who[40] = "";
            if (members) snprintf(who, sizeof(who), " of member %lld", (long long)members[(i / B) % n_m]);
            return fail(CLOTHHIP_ESTATE, "idx[%lld] = row %d%s has no old mean: call clothhip_fit_data_snapshot_policy%s or clothhip_fit_data_set_old_means on it first",
                        (long long)i, idx[i], who, members ? "_members" : "");
        }
        if (log_sigma && !h->dataset.h_old_ls_set[(size_t)idx[i]])
            return fail(CLOTHHIP_ESTATE, "idx[%lld] = row %d has no old log sigma: call clothhip_fit_data_snapshot_policy (with the head on the handle) or clothhip_fit_data_set_old_log_sigma on it first",
                        (long long)i, idx[i]);
    }
    return 0;
}
// the constants q [n_m] of a PPO call and the rows of its minibatches, after everything clothhip_policy_fit / _members refuses:
// -> tab [n_m][4], the table k_fit_loss_ppo reads. members NULL: the shared network's call, a table of one row
static int check_ppo(const clothhip_handle *h, const ClothPpoParams *q, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n_idx, int32_t B,
                     std::vector<double> *tab) {
    try { tab->resize((size_t)n_m * 4); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%d members)", n_m); }
    for (int32_t j = 0; j < n_m; j++)
        if (int rc = check_ppo_consts(q + j, members ? j : -1, tab->data() + (size_t)j * 4)) return rc;
    return check_old_set(h, members, n_m, idx, n_idx, B, false);
}

extern "C" int clothhip_policy_fit_ppo_grad(clothhip_handle *h, const ClothPpoParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out,
                                            float *ratio_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, nullptr, 1, idx, B, B, &tab)) return rc;
    return run_grad(h, policy_net(h), ppo_loss(tab.data()), SHARED_ROW, 1, idx, B, {stats_out, grad_out, ratio_out});
}

extern "C" int clothhip_policy_fit_ppo(clothhip_handle *h, const ClothFitParams *p, const ClothPpoParams *q, const int32_t *idx, int32_t n_steps, int32_t B,
                                       double *stats_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p || !q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, nullptr, 1, idx, (int64_t)n_steps * B, B, &tab)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), ppo_loss(tab.data()), p, SHARED_ROW, 1, idx, n_steps, B, {stats_out});
}

// ---- PPO for a population (clothhip.h: PPO FOR A POPULATION): the snapshot by member, and the two entries above as grouped calls ---------
// The forward of n_m members on THEIR OWN rows, scattered to the old-mean column. The rows named are grouped by member; member lists
// longer than CLOTHHIP_FIT_MAX_BATCH are cut into segments, and the k-th segments of all members that have one are launched together,
// longest first, as many as CLOTHHIP_FIT_MAX_MEMBER_ROWS holds at the longest one's length B. A shorter segment is padded to B with its
// own first row (a valid row of the same member: the layer-0 gather stays in range), which k_fit_scatter_y does not store.
struct SnapChunk { size_t m0, idx0; int32_t n_m, B; };      // offsets into the call's member / length tables and its index table
struct SnapPlan {
    std::vector<int32_t> mem, len, idx;      // per chunk member: the population row and its real positions; the index tables [n_m][B], chunk after chunk
    std::vector<SnapChunk> chunks;           // none: no row names a member
};
// the plan of rows [first, first + n) under member_of_row (every entry in [-1, pop_rows))
static int plan_snapshot(int64_t pop_rows, int64_t first, int64_t n, const int32_t *member_of_row, SnapPlan *out) {
    std::vector<int32_t> &mem = out->mem, &len = out->len, &idx = out->idx;
    try {
        // the rows of every member, ascending, as one table sorted by (member, row): start[g] .. start[g + 1]
        std::vector<int64_t> start((size_t)pop_rows + 1, 0);
        for (int64_t i = 0; i < n; i++) if (member_of_row[i] >= 0) start[(size_t)member_of_row[i] + 1]++;
        for (size_t g = 0; g < (size_t)pop_rows; g++) start[g + 1] += start[g];
        const int64_t named = start[(size_t)pop_rows];
        if (named == 0) return 0;
        std::vector<int32_t> by_member((size_t)named);
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n; i++) if (member_of_row[i] >= 0) by_member[(size_t)at[(size_t)member_of_row[i]]++] = (int32_t)(first + i);
        for (int64_t k = 0;; k++) {          // the k-th segments
            std::vector<std::pair<int32_t, int32_t>> seg;      // (length, member), longest first
            for (int64_t g = 0; g < pop_rows; g++) {
                const int64_t rest = start[(size_t)g + 1] - start[(size_t)g] - k * FIT_MAX_BATCH;
                if (rest > 0) seg.push_back({(int32_t)std::min<int64_t>(rest, FIT_MAX_BATCH), (int32_t)g});
            }
            if (seg.empty()) break;
            std::stable_sort(seg.begin(), seg.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first > b.first; });
            for (size_t s0 = 0; s0 < seg.size();) {
                const int32_t B = seg[s0].first;
                const size_t n_m = std::min<size_t>(seg.size() - s0, (size_t)(CLOTHHIP_FIT_MAX_MEMBER_ROWS / B));
                out->chunks.push_back({mem.size(), idx.size(), (int32_t)n_m, B});
                for (size_t j = s0; j < s0 + n_m; j++) {
                    const int32_t *rows = by_member.data() + start[(size_t)seg[j].second] + k * FIT_MAX_BATCH;
                    mem.push_back(seg[j].second); len.push_back(seg[j].first);
                    idx.insert(idx.end(), rows, rows + seg[j].first);
                    idx.insert(idx.end(), (size_t)(B - seg[j].first), rows[0]);
                }
                s0 += n_m;
            }
        }
    } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); }
    return 0;
}

extern "C" int clothhip_fit_data_snapshot_policy_members(clothhip_handle *h, int64_t first, int64_t n, const int32_t *member_of_row) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (int rc = check_range(h, first, n)) return rc;
    if (n == 0) return 0;
    if (!member_of_row) return fail(CLOTHHIP_EINVAL, "member_of_row is NULL");
    for (int64_t i = 0; i < n; i++)
        if (member_of_row[i] < -1 || member_of_row[i] >= h->pol.pop_rows)
            return fail(CLOTHHIP_EINVAL, "member_of_row[%lld] = %d outside [-1, %lld)", (long long)i, member_of_row[i], (long long)h->pol.pop_rows);
    auto &f = h->fit;
    const FitNet net = policy_net(h);
    const int L = net.D.n_layers;
    SnapPlan s;
    if (int rc = plan_snapshot(h->pol.pop_rows, first, n, member_of_row, &s)) return rc;
    if (s.chunks.empty()) return 0;
    HIPCHECK(hipSetDevice(h->device));
    // every chunk's scratch before the first launch: a buffer that grows is freed first
    for (const SnapChunk &c : s.chunks) if (int rc = fit_reserve(h, fit_plan(net, c.B), c.n_m)) return rc;
    if (int rc = f.d_len.reserve(s.len.size() * 4)) return rc;
    if (int rc = f.d_idx.reserve(s.idx.size() * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(f.d_len, s.len.data(), s.len.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, s.idx.data(), s.idx.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (const SnapChunk &c : s.chunks) {
        const FitPlan p = fit_plan(net, c.B);
        // (the launches read the chunk's members at the head of d_members: stream order keeps the chunks apart)
        HIPCHECK(hipMemcpyAsync(f.d_members, s.mem.data() + c.m0, (size_t)c.n_m * 4, hipMemcpyHostToDevice, h->stream));
        if (int rc = enqueue_forward(h, net, p, c.n_m, f.d_idx + c.idx0, c.B, false, policy_work(h))) return rc;
        launch_fit_scatter_y(h->stream, c.n_m, f.d_act + p.h_off[L - 1], f.d_idx + c.idx0, f.d_len + c.m0, h->dataset.old(), c.B, (int64_t)p.act);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipStreamSynchronize(h->stream));      // (the host tables the uploads read go out of scope)
    for (int64_t i = 0; i < n; i++) if (member_of_row[i] >= 0) h->dataset.h_old_set[(size_t)(first + i)] = 1;
    return 0;
}

extern "C" int clothhip_policy_fit_ppo_grad_members(clothhip_handle *h, const ClothPpoParams *q, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B,
                                                    float *grad_out, double *stats_out, float *ratio_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_m * B, B)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, members, n_m, idx, (int64_t)n_m * B, B, &tab)) return rc;
    return run_grad(h, policy_net(h), ppo_loss(tab.data()), members, n_m, idx, B, {stats_out, grad_out, ratio_out});
}

extern "C" int clothhip_policy_fit_ppo_members(clothhip_handle *h, const ClothFitParams *p, const ClothPpoParams *q, const int32_t *members, int32_t n_m,
                                               const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_fit_state(h, true)) return rc;
    if (!p || !q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_members(h, members, n_m)) return rc;
    if (int rc = check_fit_rows(h, n_m, idx, (int64_t)n_steps * n_m * B, B)) return rc;
    if (int rc = check_fit_params_members(p, n_m)) return rc;
    std::vector<double> tab;
    if (int rc = check_ppo(h, q, members, n_m, idx, (int64_t)n_steps * n_m * B, B, &tab)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), ppo_loss(tab.data()), p, members, n_m, idx, n_steps, B, {stats_out});
}

// ---- PPO with a learned sigma: one more loss mode, and the head as one more table of the optimizer (clothhip.h: PPO WITH A LEARNED SIGMA) ----
static_assert(FIT_PPO_SIGMA_STATS == CLOTHHIP_PPO_SIGMA_STATS, "the statistics of the header and of the kernel");
static_assert(sizeof(ClothPpoSigmaParams) == 16, "ClothPpoSigmaParams is two doubles");

// the constants of such a call and the rows of its minibatches, after everything clothhip_policy_fit refuses: -> the loss
static int check_ppo_sigma(const clothhip_handle *h, const ClothPpoSigmaParams *q, const int32_t *idx, int64_t n_idx, int32_t B, FitLoss *out) {
    if (!std::isfinite(q->clip) || q->clip < 0.0 || q->clip >= 1.0) return fail(CLOTHHIP_EINVAL, "clip = %g: the clip range lies in [0, 1)", q->clip);
    if (!std::isfinite(q->ent_coef) || q->ent_coef < 0.0) return fail(CLOTHHIP_EINVAL, "ent_coef = %g: the entropy coefficient is finite and >= 0", q->ent_coef);
    *out = ppo_sigma_loss(1.0 - q->clip, 1.0 + q->clip, q->ent_coef);
    return check_old_set(h, nullptr, 1, idx, n_idx, B, true);
}
static int check_head(const clothhip_handle *h) {
    if (!h->pol.has_log_sigma) return fail(CLOTHHIP_ESTATE, "no log-sigma head on this handle: call clothhip_set_policy_log_sigma first");
    return 0;
}

extern "C" int clothhip_policy_fit_ppo_sigma_grad(clothhip_handle *h, const ClothPpoSigmaParams *q, const int32_t *idx, int32_t B, float *grad_out, float *grad_ls_out,
                                                  double *stats_out, float *ratio_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_head(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    FitLoss loss;
    if (int rc = check_ppo_sigma(h, q, idx, B, B, &loss)) return rc;
    return run_grad(h, policy_net(h), loss, SHARED_ROW, 1, idx, B, {stats_out, grad_out, ratio_out, grad_ls_out});
}

extern "C" int clothhip_policy_fit_ppo_sigma(clothhip_handle *h, const ClothFitParams *p, const ClothPpoSigmaParams *q, const int32_t *idx, int32_t n_steps, int32_t B,
                                             double *stats_out, float *log_sigma_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p || !q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_fit_state(h, false)) return rc;
    if (int rc = check_head(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    FitLoss loss;
    if (int rc = check_ppo_sigma(h, q, idx, (int64_t)n_steps * B, B, &loss)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, policy_net(h), loss, p, SHARED_ROW, 1, idx, n_steps, B, {stats_out, nullptr, nullptr, nullptr, log_sigma_out});
}

extern "C" int clothhip_selftest_exp_fixed(const double *x, int64_t n, double *out) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(CLOTHHIP_EINVAL, "bad argument");
    for (int64_t i = 0; i < n; i++) {
        if (x[i] != x[i]) return fail(CLOTHHIP_EINVAL, "x[%lld] is NaN", (long long)i);
        out[i] = exp_fixed(x[i]);
    }
    return 0;
}

// ---- the critic: the value network as one more one-row table of the trainer above (clothhip.h: FITTING THE CRITIC) ------------------------
extern "C" int clothhip_value_fit_grad(clothhip_handle *h, const int32_t *idx, int32_t B, float *grad_out, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_value_state(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, B, B)) return rc;
    return run_grad(h, value_net(h), squared_error(), SHARED_ROW, 1, idx, B, {loss_out, grad_out});
}

extern "C" int clothhip_value_fit(clothhip_handle *h, const ClothFitParams *p, const int32_t *idx, int32_t n_steps, int32_t B, double *loss_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_value_state(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, (int64_t)n_steps * B, B)) return rc;
    if (int rc = check_fit_params(p, -1)) return rc;
    if (n_steps == 0) return 0;
    return run_fit(h, value_net(h), squared_error(), p, SHARED_ROW, 1, idx, n_steps, B, {loss_out});
}

extern "C" int clothhip_value_fit_reset(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit.opt_value.forget();
    return 0;
}

extern "C" int clothhip_value_predict(clothhip_handle *h, const int32_t *idx, int64_t n, float *v_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n < 1 || n > INT32_MAX) return fail(CLOTHHIP_EINVAL, "n = %lld outside [1, %d]", (long long)n, INT32_MAX);
    if (int rc = check_value_state(h)) return rc;
    if (int rc = check_fit_rows(h, 1, idx, n, (int32_t)std::min<int64_t>(n, FIT_MAX_BATCH))) return rc;
    if (!v_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    return run_predict(h, value_net(h), SHARED_ROW, 1, idx, n, v_out);
}

// ---- advantages and value targets on the device (cloth_fit_gae.hpp has the definition and the order) ------------------------------------
extern "C" int clothhip_fit_data_gae(clothhip_handle *h, int64_t first, int64_t n, const ClothGaeParams *p, float *adv_out, float *ret_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->val.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no value network on this handle: call clothhip_set_value_mlp first");
    if (int rc = check_range(h, first, n)) return rc;
    if (!p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!std::isfinite(p->gamma) || !std::isfinite(p->lambda) || !std::isfinite(p->w_scale))
        return fail(CLOTHHIP_EINVAL, "gamma %g, lambda %g, w_scale %g: all three are finite", p->gamma, p->lambda, (double)p->w_scale);
    if (p->gamma < 0.0 || p->gamma > 1.0 || p->lambda < 0.0 || p->lambda > 1.0)
        return fail(CLOTHHIP_EINVAL, "gamma %g, lambda %g: both lie in [0, 1]", p->gamma, p->lambda);
    if (p->flags & ~(CLOTHHIP_GAE_WRITE_WEIGHTS | CLOTHHIP_GAE_NORMALIZE)) return fail(CLOTHHIP_EINVAL, "unknown flags 0x%x", p->flags);
    auto &f = h->fit;
    const auto &d = h->dataset;
    for (int64_t i = 0; i < n; i++) {
        const int32_t nx = d.h_next[(size_t)(first + i)];      // (greater than first + i where it is a row: clothhip_fit_data_set_transitions)
        if (nx >= 0 && nx >= first + n)
            return fail(CLOTHHIP_EINVAL, "row %lld: its successor %d lies outside the rows [%lld, %lld + %lld)", (long long)(first + i), nx, (long long)first, (long long)first, (long long)n);
    }
    if (n == 0) return 0;
    std::vector<int32_t> idx;
    try { idx.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n); }
    for (int64_t i = 0; i < n; i++) idx[(size_t)i] = (int32_t)(first + i);
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = f.d_gae_a.reserve((size_t)n * 8)) return rc;
    if (int rc = f.d_gae_stat.reserve(16)) return rc;
    if (int rc = f.d_adv.reserve((size_t)n * 4)) return rc;
    if (int rc = enqueue_predict(h, value_net(h), SHARED_ROW, 1, idx.data(), n, nullptr)) return rc;      // (records ev0; the scan moves ev1 behind itself)
    const bool write_w = (p->flags & CLOTHHIP_GAE_WRITE_WEIGHTS) != 0, normalize = (p->flags & CLOTHHIP_GAE_NORMALIZE) != 0;
    GaeArgs a = {};
    a.v = f.d_pred; a.rew = d.rew(); a.next = d.next(); a.ret = d.ret(); a.w = d.w(); a.A = f.d_gae_a; a.adv = f.d_adv; a.stat = f.d_gae_stat;
    a.first = first; a.n = n; a.gamma = p->gamma; a.c = p->gamma * p->lambda; a.w_scale = (double)p->w_scale; a.normalize = normalize ? 1 : 0;
    const dim3 grid((unsigned)((n + GAE_THREADS - 1) / GAE_THREADS));
    hipLaunchKernelGGL(k_gae_rows, grid, dim3(GAE_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    if (write_w) {
        if (normalize) {
            hipLaunchKernelGGL(k_gae_stats, dim3(1), dim3(GAE_THREADS), 0, h->stream, a);
            HIPCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_gae_weights, grid, dim3(GAE_THREADS), 0, h->stream, a);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    if (adv_out) HIPCHECK(hipMemcpyAsync(adv_out, f.d_adv, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (ret_out) HIPCHECK(hipMemcpyAsync(ret_out, d.ret() + (size_t)first, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // (idx, a host table the upload read, goes out of scope)
    return 0;
}

// ---- DDPG: a Q critic, target networks, the deterministic policy gradient (clothhip.h: DDPG ON THE DEVICE; cloth_fit_ddpg.hpp) -------------
// Two more loss modes of the trainer above: the TD loss of the Q network, a one-row table as the value network is, over dense input rows
// X = [s, a] that k_fit_concat makes, and the policy's loss -1/B sum Q(s, clamp(mu(s))), whose dZ is the critic's input gradient. The Q
// passes work on their own scratch (FitWork), so the policy's activations survive them.
static_assert(sizeof(ClothDdpgParams) == 24, "ClothDdpgParams is two doubles, a float and an int32");
static_assert(FIT_TD_STATS + FIT_DPG_STATS == CLOTHHIP_DDPG_STATS && FIT_TD_STATS == CLOTHHIP_Q_STATS && FIT_DPG_STATS == CLOTHHIP_DPG_STATS, "the statistics of the header and of the kernels");
static_assert(FIT_NEXT_TERMINAL == CLOTHHIP_FIT_NEXT_TERMINAL, "the terminal mark of the header and of the kernel");

static FitNet q_net(clothhip_handle *h) { return {h->qnet.mlp, h->qnet.d_mlp, h->qnet.n_params, 0, h->fit.opt_q, true}; }

// What every DDPG entry refuses of the handle's state; targets: the entry reads or moves the target copies
static int check_ddpg_state(const clothhip_handle *h, bool targets, bool dataset) {
    if (int rc = check_idle(h)) return rc;
    if (h->pol.pop_rows) return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: DDPG trains the ONE shared network of clothhip_set_policy_mlp");
    if (h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    if (h->qnet.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no Q network on this handle: call clothhip_set_q_mlp first");
    if (targets && !h->tgt.policy_valid) return fail(CLOTHHIP_ESTATE, "no target policy on this handle (a new policy network drops it): call clothhip_ddpg_sync_targets first");
    if (targets && !h->tgt.q_valid) return fail(CLOTHHIP_ESTATE, "no target Q network on this handle (a new Q network drops it): call clothhip_ddpg_sync_targets first");
    if (dataset && h->dataset.n < 1) return fail(CLOTHHIP_ESTATE, "the dataset is empty: call clothhip_fit_data_append first");
    return 0;
}
static int check_tau(double tau) {
    if (!std::isfinite(tau) || tau < 0.0 || tau > 1.0) return fail(CLOTHHIP_EINVAL, "tau = %g: the soft-update rate is finite and lies in [0, 1]", tau);
    return 0;
}
static int check_ddpg_params(const ClothDdpgParams *q) {
    if (!std::isfinite(q->gamma) || q->gamma < 0.0 || q->gamma > 1.0) return fail(CLOTHHIP_EINVAL, "gamma = %g: the discount is finite and lies in [0, 1]", q->gamma);
    if (int rc = check_tau(q->tau)) return rc;
    if (!(q->act_bound > 0.0f)) return fail(CLOTHHIP_EINVAL, "act_bound = %g: the action bound is > 0 (+inf: no clamp)", (double)q->act_bound);
    if (q->flags) return fail(CLOTHHIP_EINVAL, "unknown flags 0x%x", q->flags);
    return 0;
}
// the minibatches idx [n_idx] of a DDPG call: check_fit_rows, no leaf among them -> succ (may be NULL) [n_idx], the row that holds each
// row's successor state (a terminal row: the row itself, whose value the TD kernel ignores)
static int check_ddpg_rows(const clothhip_handle *h, const int32_t *idx, int64_t n_idx, int32_t B, std::vector<int32_t> *succ) {
    if (int rc = check_fit_rows(h, 1, idx, n_idx, B)) return rc;
    if (succ) { try { succ->resize((size_t)n_idx); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%lld rows)", (long long)n_idx); } }
    for (int64_t i = 0; i < n_idx; i++) {
        const int32_t nx = h->dataset.h_next[(size_t)idx[i]];
        if (nx == CLOTHHIP_FIT_NEXT_NONE) return fail(CLOTHHIP_EINVAL, "idx[%lld] = row %d is a leaf: it has no transition (clothhip_fit_data_set_transitions)", (long long)i, idx[i]);
        if (succ) (*succ)[(size_t)i] = nx >= 0 ? nx : idx[i];
    }
    return 0;
}

static int enqueue_concat(clothhip_handle *h, bool label, const float *act, const int32_t *d_rows, int32_t B, float bound) {
    FitConcatArgs c = {};
    c.obs = h->dataset.obs(); c.lab = h->dataset.lab(); c.act = act; c.rows = d_rows; c.X = h->fit.d_qx; c.bound = bound; c.B = B; c.L = 3 * h->P;
    if (label) hipLaunchKernelGGL(k_fit_concat<true>, dim3((unsigned)B), dim3(FIT_DDPG_THREADS), 0, h->stream, c);
    else hipLaunchKernelGGL(k_fit_concat<false>, dim3((unsigned)B), dim3(FIT_DDPG_THREADS), 0, h->stream, c);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int enqueue_polyak(clothhip_handle *h, double tau) {
    const float t = (float)tau, omt = (float)(1.0 - tau);
    const int64_t n[2] = {(int64_t)h->pol.mlp_n_params, (int64_t)h->qnet.n_params};
    float *target[2] = {h->tgt.d_policy, h->tgt.d_q};
    const float *theta[2] = {h->pol.d_mlp, h->qnet.d_mlp};
    for (int k = 0; k < 2; k++) {
        hipLaunchKernelGGL(k_fit_polyak, dim3((unsigned)((n[k] + FIT_DDPG_THREADS - 1) / FIT_DDPG_THREADS)), dim3(FIT_DDPG_THREADS), 0, h->stream, target[k], theta[k], n[k], t, omt);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}
// dL/da [B][4] into h->fit.d_da from the dZ of the critic's last layer (in w.dz): the input gradients of the NN product with the mask
// epilogue down to layer 0, then layer 0's for the four action columns alone. No weight gradient is formed.
static int enqueue_action_grad(clothhip_handle *h, const FitNet &net, const FitPlan &p, int32_t B, const FitWork &w) {
    const MlpDesc &D = net.D;
    float *dz[2] = {w.dz, w.dz + (size_t)B * p.maxw};
    FitGemmArgs m0 = {};
    m0.members = h->fit.d_members; m0.stride = D.stride;
    for (int l = D.n_layers - 1; l >= 0; l--) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        FitGemmArgs b = m0;
        b.A = dz[l & 1]; b.lda = n_out;
        b.ldb = n_in; b.b_weights = 1;
        b.M = B; b.K = n_out; b.k_chunk = n_out;
        if (l > 0) {
            b.B = D.params + p.w_off[l];
            b.mask = w.act + p.h_off[l - 1];
            b.C = dz[(l - 1) & 1]; b.ldc = n_in; b.N = n_in;
            launch_gemm<true, false, FIT_EPI_MASK, false>(h->stream, b, 1);
        } else {
            b.B = D.params + p.w_off[0] + (n_in - MLP_OUT);      // W_0's action columns: the last four of a row of 3P + 4
            b.C = h->fit.d_da; b.ldc = MLP_OUT; b.N = MLP_OUT;
            launch_gemm<true, false, FIT_EPI_NONE, false>(h->stream, b, 1);
        }
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

enum { DDPG_CRITIC = 1, DDPG_ACTOR = 2, DDPG_POLYAK = 4 };
// Where a DDPG call's results go on the host, each NULL when not wanted: stats [n_steps][3 per network stepped], the critic's first; of
// a gradient call (n_steps 1, nothing updated) the one network's gradient, the critic's y [B] and q [B], the actor's dL/da [B][4]
struct DdpgOut { double *stats; float *grad, *y, *q, *da; };

// n_steps steps over idx [n_steps][B] (succ beside it, for the critic): per step the critic's (DDPG_CRITIC), the actor's against the
// critic as it stands then (DDPG_ACTOR), the soft update of both targets (DDPG_POLYAK); update false: the gradients only. The call is valid.
static int run_ddpg(clothhip_handle *h, int mode, bool update, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams &q, const int32_t *idx,
                    const int32_t *succ, int32_t n_steps, int32_t B, const DdpgOut &out) {
    auto &f = h->fit;
    const auto &d = h->dataset;
    const bool critic = (mode & DDPG_CRITIC) != 0, actor = (mode & DDPG_ACTOR) != 0;
    const FitNet pnet = policy_net(h), qnet = q_net(h);
    MlpDesc tp_desc = h->pol.mlp, tq_desc = h->qnet.mlp;
    tp_desc.params = h->tgt.d_policy; tq_desc.params = h->tgt.d_q;
    const FitNet tpnet = {tp_desc, h->tgt.d_policy, pnet.n_params, 0, f.opt_policy, false}, tqnet = {tq_desc, h->tgt.d_q, qnet.n_params, 0, f.opt_q, true};
    const FitPlan pp = fit_plan(pnet, B), qp = fit_plan(qnet, B);
    const int Lp = pnet.D.n_layers, Lq = qnet.D.n_layers, n_stats = (critic ? FIT_TD_STATS : 0) + (actor ? FIT_DPG_STATS : 0);
    const size_t n_rows = (size_t)n_steps * B, xw = (size_t)3 * h->P + MLP_OUT;
    // the step constants of both optimizers, the critic's table first; nothing of the handle changes yet
    struct Trained { const FitNet *net; const ClothFitParams *p; size_t hyper_at; } trained[2] = {};
    int n_trained = 0;
    if (update && critic) trained[n_trained++] = {&qnet, p_q, 0};
    if (update && actor) trained[n_trained++] = {&pnet, p_policy, 0};
    std::vector<float> hyper;
    try { hyper.assign((size_t)n_trained * n_steps * FIT_HYPER, 0.0f); } catch (const std::bad_alloc &) { return fail(CLOTHHIP_ENOMEM, "out of host memory (%d step constants)", n_steps); }
    for (int k = 0; k < n_trained; k++) {
        Trained &t = trained[k];
        if (!ensure_row_state(t.net->opt, 1)) return fail(CLOTHHIP_ENOMEM, "out of host memory (the optimizer's state)");
        t.hyper_at = (size_t)k * n_steps * FIT_HYPER;
        for (int s = 0; s < n_steps; s++)
            step_constants(hyper.data() + t.hyper_at + (size_t)s * FIT_HYPER, *t.p, t.p->optimizer == (float)CLOTHHIP_FIT_ADAM, t.net->opt.t[0] + s + 1);
    }
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = fit_reserve(h, pp, 1)) return rc;
    if (int rc = f.d_qx.reserve((size_t)B * xw * 4)) return rc;
    if (int rc = f.d_qact.reserve(2 * qp.act * 4)) return rc;
    if (int rc = f.d_qdz.reserve(qp.dz * 4)) return rc;
    if (qp.part) if (int rc = f.d_qpart.reserve(qp.part * 4)) return rc;
    if (int rc = f.d_qgrad.reserve(qp.grad * 4)) return rc;
    if (int rc = f.d_da.reserve((size_t)B * MLP_OUT * 4)) return rc;
    if (int rc = f.d_tdy.reserve((size_t)B * 4)) return rc;
    if (int rc = f.d_idx.reserve(n_rows * 4)) return rc;
    if (critic) if (int rc = f.d_succ.reserve(n_rows * 4)) return rc;
    if (int rc = f.d_loss.reserve((size_t)n_steps * n_stats * 8)) return rc;
    if (n_trained) if (int rc = f.d_hyper.reserve(hyper.size() * 4)) return rc;
    for (int k = 0; k < n_trained; k++) {
        if (int rc = trained[k].net->opt.m.reserve(trained[k].net->n_params * 4)) return rc;
        if (int rc = trained[k].net->opt.v.reserve(trained[k].net->n_params * 4)) return rc;
    }
    const FitWork pw = policy_work(h);
    const FitWork qw = {f.d_qact, f.d_qdz, f.d_qpart, f.d_qgrad, f.d_qx}, tqw = {f.d_qact + qp.act, nullptr, nullptr, nullptr, f.d_qx};
    // from here on the call goes through (but for a failure of the runtime itself)
    for (int k = 0; k < n_trained; k++) {
        OptState &o = trained[k].net->opt;
        if (o.zero[0]) {
            HIPCHECK(hipMemsetAsync(o.m, 0, trained[k].net->n_params * 4, h->stream));
            HIPCHECK(hipMemsetAsync(o.v, 0, trained[k].net->n_params * 4, h->stream));
            o.zero[0] = 0;
        }
        o.t[0] += n_steps;
    }
    HIPCHECK(hipMemcpyAsync(f.d_members, SHARED_ROW, 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(f.d_idx, idx, n_rows * 4, hipMemcpyHostToDevice, h->stream));
    if (critic) HIPCHECK(hipMemcpyAsync(f.d_succ, succ, n_rows * 4, hipMemcpyHostToDevice, h->stream));
    if (n_trained) HIPCHECK(hipMemcpyAsync(f.d_hyper, hyper.data(), hyper.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    const float *qv = f.d_qact + qp.h_off[Lq - 1], *y = f.d_act + pp.h_off[Lp - 1];
    float *q_dz = f.d_qdz + ((Lq - 1) & 1) * (size_t)B * qp.maxw;
    const float seed_f = -1.0f / (float)B;      // the dZ of the critic's last layer under L = -1/B sum Q
    int seed_bits;
    memcpy(&seed_bits, &seed_f, 4);
    for (int s = 0; s < n_steps; s++) {
        const int32_t *d_idx = f.d_idx + (size_t)s * B, *d_succ = f.d_succ + (size_t)s * B;
        double *st = f.d_loss + (size_t)s * n_stats;
        int k = 0;
        if (critic) {
            // the target critic on [s', clamp(mu'(s'))]: the target policy over the successor rows, on the policy's scratch
            if (int rc = enqueue_forward(h, tpnet, pp, 1, d_succ, B, false, pw)) return rc;
            if (int rc = enqueue_concat(h, false, y, d_succ, B, q.act_bound)) return rc;
            if (int rc = enqueue_forward(h, tqnet, qp, 1, nullptr, B, false, tqw)) return rc;
            // the critic on [s, clamp(a)], a the action the row executed
            if (int rc = enqueue_concat(h, true, nullptr, d_idx, B, q.act_bound)) return rc;
            if (int rc = enqueue_forward(h, qnet, qp, 1, nullptr, B, false, qw)) return rc;
            FitTdArgs t = {};
            t.q = qv; t.qn = tqw.act + qp.h_off[Lq - 1]; t.rew = d.rew(); t.next = d.next(); t.rows = d_idx; t.dz = q_dz; t.y_out = f.d_tdy; t.stats = st;
            t.gamma = q.gamma; t.B = B;
            hipLaunchKernelGGL(k_fit_loss_td, dim3(1), dim3(FIT_DDPG_THREADS), 0, h->stream, t);
            HIPCHECK(hipGetLastError());
            if (int rc = enqueue_backward(h, qnet, qp, 1, nullptr, B, qw)) return rc;
            if (update) {
                const bool adam = p_q->optimizer == (float)CLOTHHIP_FIT_ADAM;
                if (int rc = enqueue_optimizer(h, adam, qnet.theta, qnet.opt, f.d_qgrad, f.d_hyper + trained[k].hyper_at + (size_t)s * FIT_HYPER, 0, (int64_t)qnet.n_params, 1)) return rc;
                k++;
            }
            st += FIT_TD_STATS;
        }
        if (actor) {
            if (int rc = enqueue_forward(h, pnet, pp, 1, d_idx, B, false, pw)) return rc;
            if (int rc = enqueue_concat(h, false, y, d_idx, B, q.act_bound)) return rc;
            if (int rc = enqueue_forward(h, qnet, qp, 1, nullptr, B, false, qw)) return rc;
            HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)q_dz, seed_bits, (size_t)B, h->stream));
            if (int rc = enqueue_action_grad(h, qnet, qp, B, qw)) return rc;
            FitDpgArgs g = {};
            g.dA = f.d_da; g.y = y; g.q = qv; g.dz = f.d_dz + ((Lp - 1) & 1) * (size_t)B * pp.maxw; g.stats = st; g.bound = q.act_bound; g.B = B;
            hipLaunchKernelGGL(k_fit_dpg_dz, dim3(1), dim3(FIT_DDPG_THREADS), 0, h->stream, g);
            HIPCHECK(hipGetLastError());
            if (int rc = enqueue_backward(h, pnet, pp, 1, d_idx, B, pw)) return rc;
            if (update) {
                const bool adam = p_policy->optimizer == (float)CLOTHHIP_FIT_ADAM;
                if (int rc = enqueue_optimizer(h, adam, pnet.theta, pnet.opt, f.d_grad, f.d_hyper + trained[k].hyper_at + (size_t)s * FIT_HYPER, 0, (int64_t)pnet.n_params, 1)) return rc;
            }
        }
        if (mode & DDPG_POLYAK) if (int rc = enqueue_polyak(h, q.tau)) return rc;
    }
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    f.ddpg_B = B; f.ddpg_critic = critic; f.ddpg_qn_at = qp.act + qp.h_off[Lq - 1]; f.ddpg_q_at = qp.h_off[Lq - 1];
    if (out.stats) HIPCHECK(hipMemcpyAsync(out.stats, f.d_loss, (size_t)n_steps * n_stats * 8, hipMemcpyDeviceToHost, h->stream));
    if (out.grad) HIPCHECK(hipMemcpyAsync(out.grad, critic ? f.d_qgrad : f.d_grad, (critic ? qp.grad : pp.grad) * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.y) HIPCHECK(hipMemcpyAsync(out.y, f.d_tdy, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.q) HIPCHECK(hipMemcpyAsync(out.q, qv, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (out.da) HIPCHECK(hipMemcpyAsync(out.da, f.d_da, (size_t)B * MLP_OUT * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // (the host tables are never retained)
    return 0;
}

extern "C" int clothhip_q_fit_grad(clothhip_handle *h, const ClothDdpgParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out, float *y_out,
                                   float *q_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_ddpg_state(h, true, true)) return rc;
    std::vector<int32_t> succ;
    if (int rc = check_ddpg_rows(h, idx, B, B, &succ)) return rc;
    if (int rc = check_ddpg_params(q)) return rc;
    return run_ddpg(h, DDPG_CRITIC, false, nullptr, nullptr, *q, idx, succ.data(), 1, B, {stats_out, grad_out, y_out, q_out, nullptr});
}

extern "C" int clothhip_policy_fit_dpg_grad(clothhip_handle *h, const ClothDdpgParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out,
                                            float *da_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_ddpg_state(h, false, true)) return rc;
    if (int rc = check_ddpg_rows(h, idx, B, B, nullptr)) return rc;
    if (int rc = check_ddpg_params(q)) return rc;
    return run_ddpg(h, DDPG_ACTOR, false, nullptr, nullptr, *q, idx, nullptr, 1, B, {stats_out, grad_out, nullptr, nullptr, da_out});
}

// the three step entries behind their argument lists: p_policy / p_q NULL where the mode does not train that network
static int ddpg_steps(clothhip_handle *h, int mode, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams *q, const int32_t *idx,
                      int32_t n_steps, int32_t B, double *stats_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!q || ((mode & DDPG_ACTOR) && !p_policy) || ((mode & DDPG_CRITIC) && !p_q)) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(CLOTHHIP_EINVAL, "n_steps < 0");
    if (int rc = check_ddpg_state(h, mode != DDPG_ACTOR, true)) return rc;
    std::vector<int32_t> succ;
    if (int rc = check_ddpg_rows(h, idx, (int64_t)n_steps * B, B, (mode & DDPG_CRITIC) ? &succ : nullptr)) return rc;
    if (mode & DDPG_ACTOR) if (int rc = check_fit_params(p_policy, -1)) return rc;
    if (mode & DDPG_CRITIC) if (int rc = check_fit_params(p_q, -1)) return rc;
    if (int rc = check_ddpg_params(q)) return rc;
    if (n_steps == 0) return 0;
    return run_ddpg(h, mode, true, p_policy, p_q, *q, idx, succ.data(), n_steps, B, {stats_out, nullptr, nullptr, nullptr, nullptr});
}

extern "C" int clothhip_q_fit(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out) {
    return ddpg_steps(h, DDPG_CRITIC, nullptr, p, q, idx, n_steps, B, stats_out);
}

extern "C" int clothhip_policy_fit_dpg(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const int32_t *idx, int32_t n_steps, int32_t B,
                                       double *stats_out) {
    return ddpg_steps(h, DDPG_ACTOR, p, nullptr, q, idx, n_steps, B, stats_out);
}

extern "C" int clothhip_ddpg_fit(clothhip_handle *h, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams *q, const int32_t *idx,
                                 int32_t n_steps, int32_t B, double *stats_out) {
    return ddpg_steps(h, DDPG_CRITIC | DDPG_ACTOR | DDPG_POLYAK, p_policy, p_q, q, idx, n_steps, B, stats_out);
}

extern "C" int clothhip_ddpg_polyak(clothhip_handle *h, double tau) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_ddpg_state(h, true, false)) return rc;
    if (int rc = check_tau(tau)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    if (int rc = enqueue_polyak(h, tau)) return rc;
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// what the last DDPG call left in the Q passes' scratch (clothhip.h: for tests of the elementwise kernels)
extern "C" int clothhip_ddpg_last_tables(clothhip_handle *h, int32_t B, float *x_out, float *qn_out, float *q_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    auto &f = h->fit;
    if (f.ddpg_B < 1) return fail(CLOTHHIP_ESTATE, "no DDPG call has run on this handle's present Q network");
    if (B != f.ddpg_B) return fail(CLOTHHIP_EINVAL, "B = %d, the last DDPG call ran minibatches of %d rows", B, f.ddpg_B);
    if (qn_out && !f.ddpg_critic) return fail(CLOTHHIP_ESTATE, "the last DDPG call ran no critic's step: there are no target critic's values");
    HIPCHECK(hipSetDevice(h->device));
    if (x_out) HIPCHECK(hipMemcpyAsync(x_out, f.d_qx, (size_t)B * ((size_t)3 * h->P + MLP_OUT) * 4, hipMemcpyDeviceToHost, h->stream));
    if (qn_out) HIPCHECK(hipMemcpyAsync(qn_out, f.d_qact + f.ddpg_qn_at, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (q_out) HIPCHECK(hipMemcpyAsync(q_out, f.d_qact + f.ddpg_q_at, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_q_fit_reset(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    h->fit.opt_q.forget();
    return 0;
}
