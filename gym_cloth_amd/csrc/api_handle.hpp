// api_handle.hpp -- private to the api_*.hip units that implement include/clothhip.h: the handle, and the few helpers more than one of them calls.
// Each group of fields below names the one unit that writes it; a field another unit reads is read directly (the last episode launch's record: through launch_table).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "cloth_common.hpp"
#include "device_buffer.hpp"
#include "layout_plan.hpp"

using namespace clothhip;
#pragma GCC visibility push(hidden)      // the handle and the shared helpers are private to the library: nothing here reaches its dynamic symbol table

// What ONE episode launch is asked to do (api_run.hip: begin_launch; clothhip.h: clothhip_run_actions_begin has the meaning of every field).
// An optional output table is Absent, written and downloaded by _end, or written and kept on the device (want_* = 0 / 1 / 2).
enum class TableMode { Absent, Download, Keep };
enum class ResetSource { none, scripts, rng };
struct LaunchRequest {
    const ClothEpisodeParams *ep = nullptr;
    int T = 0, policy = CLOTHHIP_POLICY_TABLE;
    const double *actions = nullptr;        // [T][E][4] on the host, or on the device with actions_on_device
    bool actions_on_device = false;
    const int32_t *policy_arg = nullptr;
    ResetSource reset_source = ResetSource::none;
    const void *reset_data = nullptr;       // ClothResetScript [E][n_scripts] / the rng states uint32 [E][MT_WORDS]
    bool two_reset_sources = false;         // the public entry was given scripts AND rng states: refused in its place (check_launch)
    int n_scripts = 0, rng_tier = 0;        // (n_scripts 0 without a reset source)
    uint64_t domrand_words = 0;
    const int32_t *num_steps = nullptr;
    const uint8_t *done = nullptr;
    TableMode resets = TableMode::Absent, obs = TableMode::Absent, reset_obs = TableMode::Absent;      // (resets: never kept)
    uint64_t budget_ticks = 0;              // the time slice in 100 MHz ticks, 0: none
    // from the arming (next_request alone fills these): the expert beside the acting policy, whether it has a mix table, and whether the
    // previous launch was armed -- an action it cut left its label in EpResume
    int expert = 0;
    bool expert_mix = false, resume_labelled = false;
    bool tier2() const { return reset_source == ResetSource::rng && rng_tier == 2; }
    bool action_table() const { return policy == CLOTHHIP_POLICY_TABLE || (policy == CLOTHHIP_POLICY_MLP && actions); }      // (MLP: the optional noise table)
};

// What the last episode launch left on the device (written by api_run.hip alone; the tables themselves are EpisodeStaging's buffers).
struct LaunchRecord {
    int T = 0;                  // action slots; 0: no launch yet
    size_t reset_rows = 0;      // rows of the reset tables: E * max(n_scripts, 1)
    bool pending = false;       // between _begin and _end
    bool resets = false, rng = false;       // _end downloads reset records / the advanced rng states
    TableMode obs = TableMode::Absent, reset_obs = TableMode::Absent;
    bool armed = false;         // the label table exists (clothhip_run_actions_labels), and the label an action cut by its time slice carries over
    bool records = false;       // the record table d_frec is this launch's: false from the moment a later _begin may reallocate it
    // a _begin that has come to where the observation tables may be reallocated or overwritten: they stop being readable, whatever becomes
    // of that call; everything else the record says stays (the next launch's resume_labelled reads `armed`)
    void invalidate_obs_tables() { obs = reset_obs = TableMode::Absent; }
};
enum class LaunchTable { obs, reset_obs, labels, records };

// The columns of the trainer's dataset (clothhip_handle::FitData), each a device table of 4-byte elements, float or int32: obs [3P], the
// label [4], the loss weight, the reward, the value target, the successor row (or CLOTHHIP_FIT_NEXT_*), PPO's old mean [4] and its old log sigma [4], the expert's action [4] of DDPG from demonstrations. A column is
// described HERE and nowhere else: its width in elements per row (per_particle * P + fixed), and whether a new row gets a default -- the
// 32-bit pattern `fill` -- or is written by every append. A new column is one enumerator plus one entry, plus whatever reads it: growth,
// the defaults, clear and the range reader and writer of api_fit_data.hip are loops over this table and name no column.
enum FitCol { COL_OBS, COL_LAB, COL_W, COL_REW, COL_RET, COL_NEXT, COL_OLD, COL_OLD_LS, COL_EXP, FIT_COLS };
struct FitColDesc {
    int per_particle, fixed;
    bool defaulted;
    uint32_t fill;
    size_t width(int P) const { return (size_t)per_particle * P + fixed; }
};
constexpr FitColDesc FIT_COL[] = {
    {3, 0, false, 0},                                     // COL_OBS
    {0, 4, false, 0},                                     // COL_LAB
    {0, 1, false, 0},                                     // COL_W
    {0, 1, true, 0},                                      // COL_REW: 0.0f
    {0, 1, true, 0},                                      // COL_RET: 0.0f
    {0, 1, true, (uint32_t)CLOTHHIP_FIT_NEXT_NONE},       // COL_NEXT: no successor, a leaf
    {0, 4, true, 0},                                      // COL_OLD: zeros, and not set (FitData::h_old_set)
    {0, 4, true, 0},                                      // COL_OLD_LS: zeros, and not set (FitData::h_old_ls_set)
    {0, 4, true, 0x7fc00000u},                            // COL_EXP: four quiet NaNs, "this row has no expert action" (a row holds four finite values or four of these)
};
static_assert(sizeof(FIT_COL) / sizeof(FIT_COL[0]) == FIT_COLS, "one description per column");

// An optimizer's state, per row of the weight table it trains (max(pop_rows, 1) rows: a shared network counts as ONE row): the moments
// m, v [pop_rows][stride], [n_params] for one row (SGD's u is m), the count of steps taken and the read-as-zeros flag (the row's next
// step clears its moments first -- what a reset is, so that a reset needs no device work). Both vectors are empty until the first step
// after a new network: all rows fresh, which is what forget() makes them
struct OptState {
    Buffer<float> m, v;
    std::vector<int64_t> t;
    std::vector<uint8_t> zero;
    void forget() { t.clear(); zero.clear(); }
};

// The host fields (HostPlan: layout_plan.hpp) and everything the handle holds on its device. Each buffer frees itself; the stream and the
// events are declared in front of the buffers, so they go after them.
struct clothhip_handle : HostPlan {
    int device = 0;
    Stream stream;
    Event ev0, ev1;
    // clothhip_fork (api_state.hip): ev_fork orders a fork after the source handle's stream; the bytes of the ONE shared rest table as
    // clothhip_set_state last uploaded them (handle precision, slot order) -- the only writer of a shared table, so two shared tables are
    // equal exactly when these mirrors are; the device index lists of a fork
    struct ForkScratch {
        Event ev_fork;
        std::vector<unsigned char> shared_rest;
        Buffer<int32_t> d_fork_idx;
        PinnedBuffer<int32_t> h_fork_idx;   // (pinned staging, so that the upload is a plain DMA)
    } fork;
    ~clothhip_handle() { (void)hipSetDevice(device); }
    bool have_timing = false, pending_exec = false;
    Buffer<void> d_pos, d_prev, d_rest;
    Buffer<void> d_flat, d_flat_rest;   // flat tier-1 grid [3][Ppad] and its rest table [Spad] (window-table slot order), handle precision
    Buffer<uint8_t> d_cnt, d_active;
    int rest_stride = 0;
    Buffer<int32_t> d_tear, d_exec, d_ngrab, d_stats;
    Buffer<ClothSchedule> d_sched;
    PinnedBuffer<ClothSchedule> h_sched;   // pinned staging
    Buffer<uint32_t> d_gather, d_wt_ent;
    Buffer<unsigned long long> d_wt_dep;
    bool relaxed = false;   // clothhip_set_relaxed_order(h, 1): THIS handle's episode launches run the relaxed-order companion kernel (bench only, no parity)
    // what the next stepper launch selects and what the last one ran (api_run.hip; clothhip_set_state and clothhip_fork set lean_dirty)
    struct Launch {
        bool lean_dirty = true, lean_ok = false;   // (HostPlan::lean: the shared rest table is checked whenever it may have changed)
        int last_dispatches = 0; // kernel dispatches the last stepper launch was issued as (clothhip_last_dispatches)
        int spec_now = 0;        // 25 / 50: the layout in use runs that grid-specialised build (decided by lean_refresh per launch: spec_ns); 0: the generic build
        int last_spec = 0;       // what the last launch ran (clothhip_last_specialised)
        float pal[3] = {0, 0, 0};
        double pal64[3] = {0, 0, 0};     // fp64 LEAN build: the smallest rest length of each spring type (the others are it + a few ulps: StepArgs::lstc)
        Buffer<uint4> d_lstc;            // [Ppad] fp64 LEAN build: per particle {stencil mask, 12 offset bytes}
        int32_t last_variant[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // what the last launch ran (clothhip_last_variant)
        bool have_variant = false;
        bool on_lean = false;            // which of the two layouts runs now (lean_refresh)
        struct OccKey { const void *fn; int lds; int occ; } occ_cache[8] = {};   // hipOccupancyMaxActiveBlocksPerMultiprocessor per (kernel, LDS bytes)
    } launch;
    const Layout &lay() const { return launch.on_lean ? lay_lean : lay_std; }
    // per-env materials (clothhip_set_material): every env's effective values; how many differ bitwise from the handle's parameters (0: a uniform
    // handle -- no table goes to the kernel, the grid-specialised builds stay eligible); the device's [E] DevConsts<T> table, allocated by the first set
    std::vector<ClothMaterial> mat;
    int n_mixed = 0;
    Buffer<void> d_mat;
    Buffer<double> d_levels, d_xy, d_radius, d_cov, d_vinv;
    Buffer<uint8_t> d_oob;
    Buffer<int32_t> d_hcnt;         // per env: #points with z < thickness/2 (height reward, cloth_env.py:1047-1073)
    int n_grab_levels = 0;
    // clothhip_run_actions staging (device), sized on demand: written by clothhip_run_actions_begin / _end alone (api_run.hip). Read elsewhere:
    // last.pending (check_idle, clothhip_plan_cem); where a table of the last launch lies and how many rows it has, through launch_table below
    // (clothhip_render_obs, the row sources of api_fit_data.hip, whose gather also takes d_fobs, d_frobs, d_flab and d_frec as they are); d_frec
    // (clothhip_plan_cem); d_resume is cleared by drop_in_flight* and clothhip_fork
    struct EpisodeStaging {
        Buffer<void> d_fz, d_fact, d_fscr, d_frec, d_frst, d_fobs, d_frobs;
        Buffer<int32_t> d_fsteps, d_fparg;
        Buffer<EpResume> d_resume;      // [E] operations cut by a time slice (clothhip_run_actions), continued by the next launch
        Buffer<uint32_t> d_fmt;         // [E][MT_WORDS] numpy RandomState of every env (device-drawn resets)
        Buffer<uint8_t> d_fdone;
        Buffer<double> d_fsum;          // [E][4] per-env summary of the last episode launch (what the multi-GPU driver all-gathers)
        Buffer<uint64_t> d_fticks;      // [E][8] per-operation-class ticks and update() counts of the last episode launch
        LaunchRecord last;
        // the expert beside the acting policy: what clothhip_run_actions_expert armed for the NEXT launch (host copies of its tables) and the
        // armed launch's device tables
        int arm_expert = 0, arm_T = 0;
        bool arm_mix = false;
        std::vector<uint8_t> h_arm_mix;
        std::vector<int32_t> h_arm_choice;
        Buffer<double> d_flab;
        Buffer<uint8_t> d_fmix;
        Buffer<int32_t> d_fchoice;
    } epi;
    // clothhip_render_obs scratch (api_observe.hip) for ONE chunk of images, sized on demand: finished images (when the caller gives no device
    // buffer), raw depth, uploaded '1d' rows, valid + swap flags
    struct RenderScratch { Buffer<void> d_ro_img, d_ro_depth, d_ro_src, d_ro_flags; } ro;
    std::vector<unsigned char> stage;   // host staging for layout conversion
    std::vector<double> flat_rest;
    // The policy network and its population (api_policy.hip); outside it only mlp is read: fill_fused copies it, check_launch asks
    // whether a network exists.
    struct Policy {
        // clothhip_set_policy_mlp: the handle's network (n_layers 0: none; mlp.params = d_mlp) and clothhip_policy_eval's scratch for ONE chunk of rows
        MlpDesc mlp = {};
        Buffer<float> d_mlp, d_pe_rows;
        Buffer<double> d_pe_out;
        Buffer<int32_t> d_pl_side, d_pl_choice;   // clothhip_policy_label's per-row tables for ONE chunk (rows and results share d_pe_rows / d_pe_out)
        // clothhip_set_policy_population / clothhip_policy_population_perturb: pop_rows blobs at mlp.stride floats in d_pop (mlp.params = d_pop) and
        // the env slots' map d_member (mlp.member; its host mirror pop_member). pop_rows 0: no population (a shared network counts as ONE row for
        // clothhip_policy_eval_members and clothhip_get_policy_mlp). pop_generated: the rows were made from (pop_seed, pop_sigma, pop_flags) around row
        // pop_rows - 1 = theta, so clothhip_policy_population_combine can make the same eps again
        Buffer<float> d_pop, d_pop_center, d_pop_coef, d_pop_out;
        Buffer<int32_t> d_member, d_pe_mem;
        int64_t pop_rows = 0;
        size_t mlp_n_params = 0;
        bool pop_generated = false;
        uint64_t pop_seed = 0;
        float pop_sigma = 0.0f;
        int32_t pop_flags = 0;
        // clothhip_set_policy_log_sigma: the head of a learned standard deviation, log_sigma[4] float32 BESIDE the blob (no blob layout knows
        // it); setting or dropping a network leaves it alone, no launch reads it: the trainer's loss kernel and its optimizer do (api_fit.hip)
        Buffer<float> d_log_sigma;
        bool has_log_sigma = false;
        // clothhip_policy_noise_fill: the exploration noise double [noise_T][E][4] (noise_T 0: none), which the next episode launch may be
        // given as its device-resident table, and the uploaded sigma [rows][4] and slot_base [E] of the last fill; valid until the next
        // fill or destroy. clothhip_policy_noise_fill reads d_log_sigma where it lies.
        Buffer<double> d_noise, d_noise_sigma;
        Buffer<int64_t> d_noise_base;
        int32_t noise_T = 0;
    } pol;
    // The value network (api_policy.hip: clothhip_set_value_mlp), beside the policy and independent of it: n_layers 0: none; mlp.params =
    // d_mlp, no member map, stride 0 -- to the trainer (api_fit.hip) a weight table of ONE row. No launch evaluates it.
    struct Value {
        MlpDesc mlp = {};
        Buffer<float> d_mlp;
        size_t n_params = 0;
    } val;
    // The Q network of DDPG (api_policy.hip: clothhip_set_q_mlp), a critic over (state, action): input
    // width 3P + 4, ONE output; independent of the policy, the value network and the log-sigma head as the value network is, and to the
    // trainer one more weight table of ONE row. No launch evaluates it.
    struct QNet {
        MlpDesc mlp = {};
        Buffer<float> d_mlp;
        size_t n_params = 0;
    } qnet;
    // DDPG's target copies (api_policy.hip: clothhip_ddpg_sync_targets, _get_targets) of the shared policy blob and of the Q blob, each
    // valid from a sync until a new network of its kind (drop_network: a policy or a population; clothhip_set_q_mlp); api_fit.hip's
    // k_fit_polyak moves them
    struct DdpgTargets {
        Buffer<float> d_policy, d_q;
        bool policy_valid = false, q_valid = false;
    } tgt;
    // The device-resident dataset of the trainer and its row sources (api_fit_data.hip: clothhip_fit_data_append*, the column accessors,
    // clothhip_fit_hold, clothhip_fit_data_append_launch*). The trainer's units (fit_trainer.hpp) read the columns through the accessors below, let their kernels
    // write ret and w (clothhip_fit_data_gae) and old (clothhip_fit_data_snapshot_policy) where they lie, and read n and the mirrors.
    struct FitData {
        Buffer<uint32_t> col[FIT_COLS];      // one table per column (FIT_COL above), [cap][width], grown geometrically with the contents kept
        int64_t n = 0, cap = 0;              // rows that count, rows allocated
        float *obs() const { return (float *)col[COL_OBS]; }
        float *lab() const { return (float *)col[COL_LAB]; }
        float *w() const { return (float *)col[COL_W]; }
        float *rew() const { return (float *)col[COL_REW]; }
        float *ret() const { return (float *)col[COL_RET]; }
        int32_t *next() const { return (int32_t *)col[COL_NEXT]; }
        float *old() const { return (float *)col[COL_OLD]; }
        float *old_ls() const { return (float *)col[COL_OLD_LS]; }
        float *expert() const { return (float *)col[COL_EXP]; }
        // host mirrors [n] that grow and clear with the rows: of `next`, against which clothhip_fit_data_gae checks a range without a
        // download, and one byte per row and old column: whether its old mean / its old log sigma has been written -- against which
        // clothhip_policy_fit_ppo* (the first) and clothhip_policy_fit_ppo_sigma* (both) check a minibatch
        std::vector<int32_t> h_next;
        std::vector<uint8_t> h_old_set, h_old_ls_set;
        void mark_old_set(int64_t first, int64_t rows) { std::fill(h_old_set.begin() + first, h_old_set.begin() + first + rows, (uint8_t)1); }
        void mark_old_ls_set(int64_t first, int64_t rows) { std::fill(h_old_ls_set.begin() + first, h_old_ls_set.begin() + first + rows, (uint8_t)1); }
        // rows named by where they lie (clothhip_fit_hold, clothhip_fit_data_append_launch): held [E][3P], one row per env that outlives
        // the launch tables (held_valid: some clothhip_fit_hold has filled it); the gather's scratch: the index table of one call, its
        // not-finite flag and the weights of one clothhip_fit_data_append_launch_ex call, [n]
        Buffer<float> d_held;
        bool held_valid = false;
        Buffer<int32_t> d_rows, d_flag;
        Buffer<float> d_wtab;
    } dataset;
    // The trainer of the handle's networks (fit_trainer.hpp; api_fit.hip: clothhip_policy_fit*, clothhip_value_*; api_fit_rollout.hip:
    // clothhip_fit_data_gae, _snapshot_policy*; api_fit_ddpg.hip: clothhip_q_fit*, clothhip_policy_fit_dpg*, clothhip_ddpg_*). A new
    // network of either kind (api_policy.hip's drop_network) restarts the policy's optimizer by opt_policy.forget(), a new value network
    // the critic's by opt_value.forget(), clothhip_set_policy_log_sigma the head's by opt_sigma.forget(), a new Q network opt_q; nothing
    // else outside those three units touches it.
    struct Fit {
        // the four optimizers: the policy's, per row of its weight table, the value network's and the Q network's of ONE row each, and
        // the one of the policy's log-sigma head, a table of one row of four elements
        OptState opt_policy, opt_value, opt_sigma, opt_q;
        // The four tables the passes of one network work on, sized on demand by fit_reserve alone and handed to the launches as a
        // FitWork by fit_work alone: the hidden activations and y, the two dZ tables, the split batch sums of a weight gradient, the
        // gradient (blob layout). `own`: the trainer's, one of each per member of the call. `qpass`: the Q passes' of DDPG -- the
        // policy's activations in own survive them --, ONE of each but activations for two networks: the live critic, then the target.
        struct Pass { Buffer<float> d_act, d_dz, d_part, d_grad; } own, qpass;
        // DDPG's other scratch: the critic's input rows X [B][3P + 4], dL/da [B][4], the TD targets y [B], the successor rows of a minibatch
        Buffer<float> d_qx, d_da, d_tdy;
        Buffer<float> d_qxe;         // the BC actor's step under the Q-filter: the critic's input rows on the expert's action, X_E [B][3P + 4]
        Buffer<int32_t> d_succ;
        // what the last DDPG call left in that scratch, for clothhip_ddpg_last_tables: its B (0: nothing), whether it ran the
        // critic (the target critic's values are then there), and where in qpass.d_act the target critic's and the critic's outputs lie
        int32_t ddpg_B = 0;
        bool ddpg_critic = false;
        bool ddpg_x_expert = false;  // the last call was a BC actor's step under the Q-filter: clothhip_ddpg_last_tables' X is d_qxe
        size_t ddpg_qn_at = 0, ddpg_q_at = 0;
        // one call's tables, sized on demand: the index table, the losses; the call's member rows and its table of per-target, per-step,
        // per-member optimizer constants
        Buffer<int32_t> d_idx, d_members;
        Buffer<float> d_hyper;
        Buffer<double> d_loss;
        Buffer<float> d_pred;        // clothhip_policy_fit_predict*: y of every member and row, [n_m][n][4]; clothhip_value_predict and clothhip_fit_data_gae: v [n]
        Buffer<float> d_ratio;       // clothhip_policy_fit_ppo*_grad*: (float)rho of every member's minibatch rows, [n_m][B]
        Buffer<float> d_grad_ls, d_ls_hist;      // clothhip_policy_fit_ppo_sigma*: the head's gradient [4], the optimizer's second table; the head before every step, [n_steps][4]
        Buffer<double> d_ppo_q;      // every fixed-sigma PPO call: member j's constants {inv_s2, half_inv_s2, lo, hi} in row j, [n_m][4]; ONE row for the shared network
        Buffer<int32_t> d_len;       // clothhip_fit_data_snapshot_policy_members: the real positions of every member's index row, per chunk
        // clothhip_fit_data_gae: A of every row of the range as a double, the advantages as floats, {mean, std} of the normalisation
        Buffer<double> d_gae_a, d_gae_stat;
        Buffer<float> d_adv;
    } fit;
    // The cross-entropy planner (api_plan.hip: clothhip_plan_cem on the SCRATCH handle, clothhip_plan_sample / _refit on the handle given), all
    // sized on demand: the distribution d_mean, d_std [E][H][4], the best so far d_best_a [E][H][4], d_best_s [E], the source's done flags, the
    // action tables d_x [H][E K][4] (one, or one per iteration when the caller wants them back), d_scores [n_iters][E][K], the elite flags and
    // top indices of the stand-alone refit
    struct Plan {
        Buffer<double> d_mean, d_std, d_best_a, d_best_s, d_x, d_scores;
        Buffer<uint8_t> d_done, d_elite;
        Buffer<int32_t> d_top;
    } plan;
};

// f(float{}) or f(double{}) by the handle's precision: a launch that exists in both precisions is written once, as a generic lambda
template <typename F> static auto by_precision(const clothhip_handle *h, F &&f) { return h->precision == CLOTHHIP_F64 ? f(double{}) : f(float{}); }

// The helpers more than one unit calls, each defined in the unit named
namespace clothhip {
int check_params(const ClothParams *p);                                                          // api_core.hip
int check_idle(const clothhip_handle *h);
int check_range(const clothhip_handle *h, int64_t first, int64_t n);                             // api_fit_data.hip: rows [first, first + n) lie within the dataset
// api_fit_data.hip, the one includer of cloth_fit_gather.hpp, for the trainer: that header's k_fit_sqsum over one block and k_fit_copy_y over
// blocks * n_m, argument for argument
void launch_fit_sqsum(hipStream_t s, const float *y, const float *lab, const float *wgt, const int32_t *rows, int32_t B, double *sum);
void launch_fit_copy_y(hipStream_t s, int32_t n_m, const float *y, int32_t n_vals, float *out, int64_t y_step, int64_t out_step, int32_t blocks);
// ... and k_fit_scatter_y over n_m members of B positions each, len[j] of them real
void launch_fit_scatter_y(hipStream_t s, int32_t n_m, const float *y, const int32_t *rows, const int32_t *len, float *col, int32_t B, int64_t y_step);
int check_material(const ClothParams &prm, const ClothMaterial &m, int idx);                     // api_state.hip
SpecPhys phys_of(const ClothParams &p);
SpecPhys phys_of(const ClothParams &p, const ClothMaterial &m);
ClothMaterial material_of(const ClothParams &p);
int drop_in_flight(clothhip_handle *h, const uint8_t *d_mask, const ClothSchedule *d_sched);
int plan_steppers(clothhip_handle *h);                                                           // api_run.hip, for clothhip_create
LaunchRequest next_request(clothhip_handle *h);      // api_run.hip: an empty request for h's next launch; TAKES the arming, which is gone whatever becomes of the request
int begin_launch(clothhip_handle *h, const LaunchRequest &req);                                  // api_run.hip: clothhip_run_actions_begin behind its argument list
int run_actions_end_on_device(clothhip_handle *h);                                               // api_run.hip, for clothhip_plan_cem
// api_run.hip: where a table of the last launch lies and its rows ([T * E], reset_obs [E * n_scripts]; either result may be NULL), or
// CLOTHHIP_ESTATE when the record says it is not there. Does not ask whether a launch is in flight: check_idle
int launch_table(const clothhip_handle *h, LaunchTable which, const void **d_ptr, int64_t *rows);
}  // namespace clothhip
#pragma GCC visibility pop
