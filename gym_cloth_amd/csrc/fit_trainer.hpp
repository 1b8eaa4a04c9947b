// fit_trainer.hpp -- private to the trainer's units (api_fit.hip, api_fit_rollout.hip, api_fit_ddpg.hip): what a call trains, where its tables
// lie, what it minimises, which tables its optimizer steps, and the launches and checks of api_fit.hip that the other two call. Every
// function declared here is defined in api_fit.hip, the one unit that includes the trainer's kernel headers.
#pragma once
#include <vector>

#include "api_handle.hpp"
#include "cloth_policy_mlp.hpp"

#pragma GCC visibility push(hidden)

extern const int32_t SHARED_ROW[1];            // the member list of the shared network, and of the value and the Q network

// The weight table a call trains, and what belongs to it: the policy's (shared network or population), the value network's or the Q
// network's one row.
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
FitNet policy_net(clothhip_handle *h);
FitNet value_net(clothhip_handle *h);

// What the entries refuse before anything is touched, each in the order it always had (api_fit.hip has the meaning of every argument)
int check_fit_state(const clothhip_handle *h, bool population);
int check_value_state(const clothhip_handle *h);
int check_fit_rows(const clothhip_handle *h, int32_t n_m, const int32_t *idx, int64_t n_idx, int32_t B);
int check_fit_params(const ClothFitParams *p, int32_t j);

// Where member j's tables lie: the per-member sizes of the scratch tables (floats) for minibatches of B rows, and the offsets of every
// layer inside a blob (weights, gradient) and inside a member's activations.
struct FitPlan {
    size_t act, dz, part, grad, maxw;       // per member: activations, the two dZ tables, the slabs (0 without a split), the gradient
    int n_split;
    size_t w_off[MLP_MAX_LAYERS], h_off[MLP_MAX_LAYERS];
};
FitPlan fit_plan(const MlpDesc &D, int32_t B);
// one step's scratch in t: gradients, dZ tables and slabs for n_grad members, activations for n_act passes
int fit_reserve(clothhip_handle::Fit::Pass &t, const FitPlan &p, size_t n_grad, size_t n_act);
// ... the trainer's own for n_m members, and the call's member table
int fit_reserve(clothhip_handle *h, const FitPlan &p, int32_t n_m);

// The tables a pass of one network works on: its activations, the two dZ tables, the slabs of a split batch sum, the gradient (each
// NULL where the pass does not touch it), and its layer-0 input -- x NULL: the dataset's observation rows through the call's index
// table, else dense rows [B][widths[0]] (the critic's [s, a] rows of DDPG). Valid after fit_reserve of that instance.
struct FitWork { float *act, *dz, *part, *grad; const float *x; };
FitWork fit_work(const clothhip_handle::Fit::Pass &t, const float *x = nullptr);

// What a step minimises, with the fields that loss reads and no others. The width of the squared error comes from FitNet; both
// surrogates, DPG and DPG_BC are the policy's table only, TD the Q network's. A new loss is one more kind, its fields, and its case in enqueue_loss.
struct FitLoss {
    enum Kind { SQUARED_ERROR, PPO, PPO_SIGMA, TD, DPG, DPG_BC } kind;
    int stats;                                      // doubles per member and step in the loss table: the loss, or the loss's statistics
    union {
        const double *q;                            // PPO: host [n_m][4] {inv_s2, half_inv_s2, lo, hi}, row j member j's (check_ppo makes it)
        struct { double lo, hi, ent_coef; } s;      // PPO_SIGMA: 1 - eps, 1 + eps and the entropy coefficient; 1 / sigma^2 comes from the head
        struct { const float *qn; float *y_out; double gamma; } td;      // TD: the target critic's values [B], where y [B] goes, the discount
        struct { const float *dA, *q; float bound; } dpg;                // DPG: dL/da [B][4], the critic's output this pass [B], the action bound
        struct { const float *dA, *q, *qe; float bound, qc, bc; } bc;    // DPG_BC: DPG's, the critic on the expert's action [B] (NULL: no Q-filter), q_coef and bc_coef
    };
};
FitLoss td_loss(const float *qn, float *y_out, double gamma);
FitLoss dpg_loss(const float *dA, const float *q, float bound);
FitLoss dpg_bc_loss(const float *dA, const float *q, const float *qe, float bound, float qc, float bc);

// Where a call's results go on the host, each NULL when the caller does not want it: loss [n_steps][n_m][stats]; of a gradient call grad
// [n_m][n_params], ratio [n_m][B] (the surrogates), grad_ls [4] (PPO_SIGMA); of a PPO_SIGMA fit ls [n_steps][4], the head before each update
struct FitOut { double *loss; float *grad, *ratio, *grad_ls, *ls; };

// The launches of one network's step, each over all n_m members (api_fit.hip)
int enqueue_forward(clothhip_handle *h, const MlpDesc &D, const FitPlan &p, int32_t n_m, const int32_t *d_idx, int32_t B, bool shared_rows, const FitWork &w);
int enqueue_loss(clothhip_handle *h, const FitNet &net, const FitPlan &p, const FitLoss &loss, int32_t n_m, const int32_t *d_idx, int32_t B, double *d_stats,
                 float *d_ratio, float *d_ls, const FitWork &w);
int enqueue_backward(clothhip_handle *h, const MlpDesc &D, const FitPlan &p, int32_t n_m, const int32_t *d_idx, int32_t B, const FitWork &w);
int enqueue_action_grad(clothhip_handle *h, const MlpDesc &D, const FitPlan &p, int32_t B, const FitWork &w);
int enqueue_predict(clothhip_handle *h, const FitNet &net, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *dst);
// cloth_fit_ddpg.hpp's k_fit_concat and k_fit_polyak, and cloth_policy_fit.hpp's k_fit_fill_ls over n4 floats
int enqueue_concat(clothhip_handle *h, bool label, const float *act, const int32_t *d_rows, int32_t B, float bound);
int enqueue_concat_expert(clothhip_handle *h, const int32_t *d_rows, int32_t B, float bound);      // k_fit_concat's expert mode, into h->fit.d_qxe
int enqueue_polyak(clothhip_handle *h, double tau);
int enqueue_fill_ls(clothhip_handle *h, float *dst, int64_t n4);

// One table the optimizer steps in a call: the rows `members` [n_m] of theta, n elements each at members[j] * stride, with the moments
// and step counts of `opt`; row j's gradient lies at grad + j * n, and its step constants are made from p[j] -- Adam or SGD by p[0].
struct OptTarget {
    float *theta;
    OptState *opt;
    size_t rows, moments;               // rows of the whole table; floats of each moment table
    int64_t stride, n;
    const int32_t *members;             // host
    int32_t n_m;
    const Buffer<float> *grad;          // (a pointer only after the call's reserves)
    const ClothFitParams *p;
    size_t hyper_at;                    // where its constants lie in the call's table (opt_prepare)
};
OptTarget net_target(const FitNet &net, const int32_t *members, int32_t n_m, const Buffer<float> &grad, const ClothFitParams *p);
// The targets of one call, in the order of their step constants: ONE table [target][step][its n_m][FIT_HYPER], on the host and in d_hyper.
// None: the call updates nothing, reserves no moments and uploads no constants.
struct OptPlan {
    OptTarget t[2];
    int n = 0;
    int32_t n_steps = 0;
    std::vector<float> hyper;
    void add(const OptTarget &x) { t[n++] = x; }
};
// The phases of a call, in this order: host-only preparation that can fail and changes nothing of the handle (every row's state exists,
// the step constants); the reserves (d_hyper, both moment tables of every target); the commit, from which on the call goes through
// (first-touch zeroing of the moments, the step counts, the upload of the constants); and step s of target k
int opt_prepare(OptPlan &o, int32_t n_steps);
int opt_reserve(clothhip_handle *h, const OptPlan &o);
int opt_commit(clothhip_handle *h, OptPlan &o);
int enqueue_optimizer(clothhip_handle *h, const OptPlan &o, int k, int s);

#pragma GCC visibility pop
