/*
 * clothhip.h -- C ABI of libclothhip.so, the MI355X (gfx950) cloth stepper.
 *
 * Drop-in boundary for the hot path of DanielTakeshi/gym-cloth: the Python object API of the three
 * Cython modules gym_cloth/physics/{cloth,point,gripper}.pyx that ClothEnv imports at
 * gym_cloth/envs/cloth_env.py:25-27.  The reference has no FFI layer of its own; these entry points
 * are what a ctypes binding for that path binds (INTEGRATION.md shows the stub).  Every entry point
 * names the reference interface it replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - plain C types only; host arrays are caller-owned, passed as pointer + explicit extents, never
 *     retained after the call returns.
 *   - E = n_envs of the handle, P = n_side*n_side points, S = clothhip_num_springs() springs.
 *   - host position arrays are [E][P][3] doubles (x,y,z interleaved) = E stacked Cloth.allpts_arr
 *     (cloth.pyx:395); the device keeps SoA [E][3][Ppad] in the handle's precision.
 *   - every call returns 0 on success or a negative CLOTHHIP_E* code; clothhip_last_error() gives a
 *     thread-local message.  No C++ exception and no abort() crosses the ABI.
 *   - calls on one handle are not re-entrant.  Calls enqueue on the handle's HIP stream and
 *     synchronise before returning unless the name ends in _async.
 *   - there is NO CPU fallback: without a HIP device clothhip_create fails with CLOTHHIP_ENODEV.
 */
#ifndef CLOTHHIP_H
#define CLOTHHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLOTHHIP_ABI_VERSION 7

enum {
    CLOTHHIP_OK = 0,
    CLOTHHIP_EINVAL = -1,   /* bad argument (ValueError / AssertionError in the reference, cloth.pyx:85,91,132) */
    CLOTHHIP_ENODEV = -2,   /* no usable HIP device */
    CLOTHHIP_EHIP = -3,     /* a HIP runtime call failed; message has the hipError string */
    CLOTHHIP_ENOMEM = -4,   /* out of host or device memory: any HIP call that reports hipErrorOutOfMemory, whichever buffer ran out -- the fixed
                               ones of clothhip_create and clothhip_set_material as well as the ones a call sizes by its arguments (episode
                               launches, render, fork) */
    CLOTHHIP_ESTATE = -5    /* call not valid in the handle's current state */
};

enum { CLOTHHIP_F64 = 0, CLOTHHIP_F32 = 1 };

/* clothhip_set_state flags */
enum {
    CLOTHHIP_REST_SHARED = 1,   /* `rest` is ONE [S] table used by all envs of the handle (tiers 1 and 3) */
    CLOTHHIP_KEEP_TEAR = 2      /* do not clear Cloth.cloth_have_tear (it is sticky in the reference, cloth.pyx:272-273):
                                   for position writes into a live cloth (pts[i].x = ..., Gripper.adjust) as opposed to
                                   the Cloth(...) rebuild of a reset */
};

/* Physics constants: the keys Cloth.__init__/Cloth.update read from the cfg dict
 * (cloth.pyx:53-56, :175-186) plus the Cloth() constructor defaults (cloth.pyx:24-26) and the
 * Gripper constructor arguments (gripper.pyx:10; cloth_env.py:752-753). */
typedef struct ClothParams {
    int32_t n_side;            /* cloth.num_width_points == cloth.num_height_points (asserted, cloth.pyx:91) */
    int32_t frames_per_sec;    /* cfg frames_per_sec */
    int32_t simulation_steps;  /* cfg simulation_steps */
    int32_t _pad;
    double width, height;      /* cfg cloth.width / cloth.height */
    double density, ks, damping, thickness, plane_friction, tear_thresh;  /* cfg cloth.* */
    double gravity;            /* Cloth(gravity=-9.8) */
    double minimum_z;          /* Cloth(minimum_z=0)  */
    double grip_radius;        /* cfg env.grip_radius (default Gripper.grip_radius) */
} ClothParams;

/* One pick-and-place schedule = the hot loop of ClothEnv.step + ClothEnv._pull
 * (cloth_env.py:352-367, :472-515):
 *   for i in [0, n_total):
 *       i <  n_up_end       : gripper.adjust(0, 0, dz_up)
 *       i <  n_uprest_end   : -
 *       i <  n_pull_end     : gripper.adjust(dx_pull, dy_pull, dz_pull)   (dz_pull = 0 in the reference)
 *       i <  n_griprest_end : -
 *       else                : gripper.release()
 *       cloth.update()
 *       if break_on_tear and cloth.have_tear: break
 * The n_* are the integer ceilings of the reference's cumulative (possibly fractional: tier 3 draws a
 * float iters_up, cloth_env.py:960) phase boundaries, so `i < boundary` is unchanged.
 * A raw `for _ in range(n): cloth.update()` is {0,0,0,n,n}, break_on_tear=0. */
typedef struct ClothSchedule {
    int32_t n_up_end, n_uprest_end, n_pull_end, n_griprest_end, n_total;
    int32_t break_on_tear;
    int32_t active;            /* 0: this env is skipped entirely (cloth_env.py:490-493 "nothing grabbed") */
    int32_t _pad;
    double dz_up;              /* 0.0025 in the reference (cloth_env.py:359) */
    double dx_pull, dy_pull;   /* x_dir_r, y_dir_r (cloth_env.py:455-456) */
    double dz_pull;            /* 0 in the reference (cloth_env.py:363); lets clothhip_update pass any delta */
} ClothSchedule;

typedef struct clothhip_handle clothhip_handle;

const char *clothhip_last_error(void);
int clothhip_abi_version(void);
/* number of visible HIP devices (0 if none / runtime unusable); never fails */
int clothhip_device_count(void);

/* Replaces Cloth(...) + Gripper(...) construction for a batch of E independent cloths
 * (cloth.pyx:23-167, gripper.pyx:10-21; cloth_env.py:737-753). State starts as the flat tier-1 grid. */
int clothhip_create(const ClothParams *params, int32_t n_envs, int32_t device, int32_t precision,
                    clothhip_handle **out);
int clothhip_destroy(clothhip_handle *h);
int clothhip_num_points(const clothhip_handle *h);
int clothhip_num_springs(const clothhip_handle *h);
int clothhip_num_envs(const clothhip_handle *h);
int clothhip_precision(const clothhip_handle *h);

/* Host-side restatement of the grid/spring construction of Cloth.__init__ (cloth.pyx:92-146, :411-417),
 * in double, for one cloth: fills pos[P][3] and rest[S]. tier 1/3 = flat grid, tier 2 = vertical sheet
 * with the P np_random.rand() draws passed in rand_draws (r-major order). Pure host function. */
int clothhip_init_grid(const ClothParams *params, int32_t tier, int32_t init_side,
                       const double *rand_draws, double *pos, double *rest);
/* Spring list (ptA index, ptB index, type 0/1/2 = STRUCTURAL/SHEARING/BENDING) in reference list order. */
int clothhip_spring_topology(const ClothParams *params, int32_t *a, int32_t *b, uint8_t *type);

/* State upload/download for envs [env0, env0+n): the replacement for writing/reading
 * pts[i].x/.y/.z/.px/.py/.pz/.pinned (point.pyx:34-48; read at cloth_env.py:196-200, :629, :854-937).
 * Any pointer may be NULL (= leave untouched / do not fetch).  rest is [n][S] (Spring.rest_length), or with
 * CLOTHHIP_REST_SHARED in `flags` a single [S] table used by ALL envs of the handle (tier 1/3).
 * pinned != 0 marks the point pinned and a member of gripper.grabbed_pts. set_state clears the tear flag
 * of the envs it touches when `pos` is given, unless CLOTHHIP_KEEP_TEAR is set. */
int clothhip_set_state(clothhip_handle *h, int32_t env0, int32_t n, const double *pos, const double *prev,
                       const uint8_t *pinned, const double *rest, int32_t flags);
int clothhip_get_state(clothhip_handle *h, int32_t env0, int32_t n, double *pos, double *prev,
                       uint8_t *pinned);
/* Spring.rest_length (cloth.pyx:417) of envs [env0, env0+n) in reference list order: rest[n][S]
 * (what the reference's save_state pickle keeps per spring, cloth_env.py:343-350). */
int clothhip_get_rest(clothhip_handle *h, int32_t env0, int32_t n, double *rest);
/* The Cloth(...) rebuild of ClothEnv.reset (cloth_env.py:737-746) for the flat tiers 1 and 3, on the device:
 * every env with mask[e] != 0 (mask NULL = all) gets the flat grid (cloth.pyx:117-130) as position and previous
 * position, nothing pinned, tear flag cleared, flat rest lengths. No host upload. */
int clothhip_reset_flat(clothhip_handle *h, const uint8_t *mask);
/* Cloth.have_tear (cloth.pyx:390-392) for every env: tear[E] (0/1). set: overwrite (Cloth() is rebuilt
 * per reset in the reference, which clears it). */
int clothhip_get_tear(clothhip_handle *h, uint8_t *tear);
int clothhip_set_tear(clothhip_handle *h, const uint8_t *tear);

/* Per-env MATERIAL: the six quantities of ClothParams that describe the fabric and its world but not the grid. The reference reads them
 * from the cfg in every Cloth.update() call (cloth.pyx:175-186: density -> mass and mass * gravity, ks, damping, plane_friction; used at
 * :240-241 (Verlet: (dt*dt)/mass, 1 - damping/100), :368 (1. - plane_friction) and :272 (tear_thresh)), so they are ordinary inputs per
 * cloth: one handle may step cloths of different fabrics. Everything else of ClothParams stays per handle (grid, thickness, rates, ...). */
typedef struct ClothMaterial { double density, ks, damping, plane_friction, tear_thresh, gravity; } ClothMaterial;
/* Give envs [env0, env0+n) the materials m[n]; m NULL: these envs go back to the handle's ClothParams. A material belongs to the env
 * SLOT: set_state, reset_flat, the resets inside an episode launch and the parked operations of a time-sliced launch keep it; only this
 * call changes it. Values follow the rules clothhip_create applies to these fields (density > 0): a bad value or range returns
 * CLOTHHIP_EINVAL and changes nothing. CLOTHHIP_ESTATE between clothhip_run_actions_begin and _end. Touches neither the particle state nor
 * the operations in flight. While any env's material differs bitwise from the handle's parameters the handle runs the generic stepper
 * build (clothhip_last_specialised reports 0), which reads every env's constants from a device table; without one it runs exactly the
 * kernels and the bits it runs without this call. With clothhip_set_relaxed_order on, such a handle gets CLOTHHIP_ESTATE from
 * clothhip_run_actions* (the companion kernel is bench-only). */
int clothhip_set_material(clothhip_handle *h, int32_t env0, int32_t n, const ClothMaterial *m);
/* The effective materials of envs [env0, env0+n) into m[n] (the handle's parameters for envs never given one). */
int clothhip_get_material(clothhip_handle *h, int32_t env0, int32_t n, ClothMaterial *m);
/* Host only: the seven stepper constants a material turns into on a handle of `params` and `precision` (m NULL: the handle's own), by the
 * one derivation the kernels' constants come from, widened to double: out = {mass * gravity, ks * 1.0, ks * 0.2, (dt*dt)/mass,
 * 1 - damping/100, 1. - plane_friction, tear_thresh}. */
int clothhip_selftest_material(const ClothParams *params, const ClothMaterial *m, int32_t precision, double out[7]);

/* Whole cloths from env slot to env slot, ON THE DEVICE: destination env dst_env[j] of `dst` becomes a copy of env src_env[j] of `src`, j in
 * [0, n). Replaces the host round trip clothhip_get_state -> clothhip_set_state (+ get_tear / get_rest / get_material and their setters) for
 * branching one state into many (action lookahead), keeping a state and coming back to it (snapshot / restore) and starting every env from
 * one state -- what the reference does with save_state / Cloth(state=...) through a pickle (cloth_env.py:343-350, :736-741). One kernel on
 * dst's stream copies, bit for bit and without conversion: positions and previous positions, the per-point pin bytes VERBATIM (the grab
 * multiplicity clothhip_get_state collapses to 0/1 and the pinned-from-outside bit of clothhip_pin_points, which it hides), the tear flag
 * (copied, not cleared) and, unless CLOTHHIP_FORK_STATE_ONLY, the material. The launch waits for what src's stream has enqueued (an event)
 * and the call returns when the copy is done.
 *   - dst and src: same device, precision and n_side, else CLOTHHIP_EINVAL; dst == src is allowed when no env is in both lists.
 *     CLOTHHIP_EINVAL also for an index out of range, a duplicate in dst_env, or an env that is source and destination on one handle; a
 *     duplicate in src_env is the point (one state, many branches). n == 0 succeeds and does nothing. A failed call changes nothing.
 *     CLOTHHIP_ESTATE between clothhip_run_actions_begin and _end on either handle.
 *   - like clothhip_set_state, the fork drops the operation a time slice left in flight -- for the destination envs it writes, only;
 *     the source's parked operations are neither copied nor disturbed.
 *   - rest lengths: afterwards clothhip_get_rest of a destination env equals its source env's bit for bit. A destination that shares ONE
 *     rest table keeps sharing it when the source shares a bitwise-equal one (the flat tiers keep their LEAN and grid-specialised builds).
 *     Equality is decided on the host without a download: clothhip_set_state with CLOTHHIP_REST_SHARED is the only writer of a shared table
 *     (the kernels write rest lengths into per-env tables only), every handle keeps the bytes it last uploaded that way, in its precision,
 *     and two shared tables are equal exactly when those bytes are. In every other case the destination switches to per-env tables (its
 *     other envs keep their values), as clothhip_set_state does when given per-env `rest`, and the source env's row is copied.
 *   - materials: without CLOTHHIP_FORK_STATE_ONLY the destination envs take their source envs' ClothMaterial by clothhip_set_material's
 *     rules (the handle's material table, the generic build while any env differs from the handle's parameters, clothhip_last_specialised
 *     following); with the flag they keep their own. */
enum { CLOTHHIP_FORK_STATE_ONLY = 1 };   /* leave the destination envs' materials as they are */
int clothhip_fork(clothhip_handle *dst, const int32_t *dst_env, clothhip_handle *src, const int32_t *src_env,
                  int32_t n, int32_t flags);
/* The raw per-point pin byte of envs [env0, env0+n): cnt[n][P], bits 0-6 = how many times the gripper holds the point (grabbed_pts may
 * list a point more than once, gripper.pyx:41,52), bit 7 = pinned from outside (clothhip_pin_points). clothhip_get_state's `pinned` is
 * this byte != 0. */
int clothhip_get_pin_counts(clothhip_handle *h, int32_t env0, int32_t n, uint8_t *cnt);
/* parked[E]: 1 for every env that holds an operation a time-sliced clothhip_run_actions launch cut and the next launch would continue
 * (see time_budget_ms there), else 0. A fork, a snapshot or a lookahead of such an env would copy a cloth in the middle of an action
 * without the action's remainder: callers take them between whole actions and ask here. */
int clothhip_in_flight(clothhip_handle *h, uint8_t *parked);

/* Gripper.grab_top(x, y) (gripper.pyx:23-42) for every active env: xy[E][2]; radius[E] or NULL
 * (= params.grip_radius; cloth_env.py:436-442 mutates it for force_grab); active[E] or NULL (= all).
 * n_grabbed[E] receives the number of points appended to grabbed_pts by THIS call (0 = nothing grabbed). */
int clothhip_grab_top(clothhip_handle *h, const double *xy, const double *radius, const uint8_t *active,
                      int32_t *n_grabbed);
/* Gripper.grab(x, y) (gripper.pyx:44-53) */
int clothhip_grab(clothhip_handle *h, const double *xy, const double *radius, const uint8_t *active,
                  int32_t *n_grabbed);
/* Gripper.release() (gripper.pyx:68-73) */
int clothhip_release(clothhip_handle *h, const uint8_t *active);
/* pt.pinned = True from outside the gripper (point.pyx:48 is a plain writable attribute): idx[n] point
 * indices of env `env`; the points are pinned but NOT members of grabbed_pts (adjust does not move them). */
int clothhip_pin_points(clothhip_handle *h, int32_t env, const int32_t *idx, int32_t n);

/* The hot path. Runs sched[e] for every env e (see ClothSchedule) entirely on the device:
 * n_total x { Gripper.adjust / release ; Cloth.update (cloth.pyx:169-214) ; tear break }.
 * executed[E] (may be NULL) receives the number of update() calls each env performed. */
int clothhip_run(clothhip_handle *h, const ClothSchedule *sched, int32_t *executed);
int clothhip_run_async(clothhip_handle *h, const ClothSchedule *sched);
/* wait for the handle's stream; after an _async call also fetches executed[E] (may be NULL) */
int clothhip_sync(clothhip_handle *h, int32_t *executed);

/* ---- Whole episodes on the device -------------------------------------------------------------------------------
 * clothhip_run_actions runs T consecutive ClothEnv.step calls (cloth_env.py:369-534) for every env in ONE launch, with
 * the particle state resident on the CU: action source (table or scripted policy), the action -> schedule arithmetic
 * (:396-475), Gripper.grab_top (+ force_grab, :434-444), the hot loop (:495-515), the per-action metrics
 * (:1020-1098), the terminal test (:684-715) and -- when a reset script is supplied -- the ClothEnv.reset of an env whose
 * episode ended (:717-987, tiers 1 and 3), i.e. the reference's episode loop `while not done: step` / `env.reset()`
 * (examples/analytic.py:872-882) without a host round trip. Envs never wait for each other inside the launch.
 * Reward and info bookkeeping stay on the host (gym_cloth_amd/envs.py::ClothVecEnv.step_many) and are computed from the
 * records below. */

/* constants of ClothEnv.__init__ / step / _terminal the device needs (cloth_env.py:87-186) */
typedef struct ClothEpisodeParams {
    int32_t max_actions;             /* env.max_actions */
    int32_t iters_up_rest, iters_grip_rest, iters_rest;
    int32_t clip_act_space;          /* env.clip_act_space */
    int32_t force_grab;              /* env.force_grab */
    int32_t _pad[2];
    double iters_up;                 /* env.iters_up (tier 3 overrides it per reset pull with a float, cloth_env.py:960) */
    double reduce_factor, grip_radius;
    double radius_inc;               /* 0.02, cloth_env.py:131 */
    double dz_up;                    /* 0.0025, cloth_env.py:359 */
    double act_low[4], act_high[4];  /* action_space.low / .high (cloth_env.py:162-181) */
    double coverage_done;            /* _REWARD_THRESHOLDS[reward_type] (cloth_env.py:42-50, :706) */
} ClothEpisodeParams;

enum { CLOTHHIP_POLICY_TABLE = 0,          /* actions[t][e][4] given by the caller (any policy run on the host, or random) */
       CLOTHHIP_POLICY_ORACLE_CORNER = 1,  /* examples/analytic.py:105-155, 'distance' method, delta actions, 25x25 only */
       CLOTHHIP_POLICY_HIGHEST_POINT = 2,  /* examples/analytic.py:723-808: the k-th highest point (stable order), pulled to where it
                                              sits on the flat cloth; k per slot and env from policy_arg (the reference draws it
                                              with np.random.randint(top_k = 5)) */
       CLOTHHIP_POLICY_MLP = 3             /* the handle's network (clothhip_set_policy_mlp) on the cloth's '1d' observation at the start of
                                              the slot, + actions[t][e][4] where `actions` is given (no reference counterpart) */ };

/* One scripted pull of a reset (cloth_env.py:851-877 tier 1, :959-978 tier 3): the raw RNG draws; everything that
 * depends on the particle state (the picked point's position, _prevent_oob) is evaluated on the device. */
typedef struct ClothResetPull {
    int32_t point;                   /* >= 0: pick at pts[point] (tier 1: np_random.randint(P)); < 0: pick at (x, y) */
    int32_t need_coverage;           /* bit 0: run this pull (and the later ones) only if coverage >= coverage_min (tier 1's 3rd);
                                        bit 1: do not apply _prevent_oob (tier 2's pulls, cloth_env.py:905-947) */
    double x, y;                     /* pick point when point < 0 (tier 3: p0x, p0y) */
    double dx, dy;                   /* drawn deltas BEFORE _prevent_oob (cloth_env.py:834-840, applied on the device) */
    double iters_up;                 /* iters_up of this pull (tier 3: uniform(200, 280); else env.iters_up) */
    double coverage_min;             /* 0.90 (cloth_env.py:866) */
} ClothResetPull;

typedef struct ClothResetScript {
    int32_t valid;                   /* 0: no script in this slot */
    int32_t n_pulls;                 /* <= 3 */
    int32_t settle_after;            /* bare update() calls after the pulls (tier 3: 800, cloth_env.py:980-981) */
    int32_t _pad;
    ClothResetPull pull[3];
} ClothResetScript;

/* what happened in action slot t of env e */
typedef struct ClothStepRecord {
    double action[4];                /* the action taken, as passed to step() (clip space if clip_act_space) */
    double coverage, variance_inv;   /* after the action (cloth_env.py:1075-1098) */
    int32_t executed;                /* update() calls of this action (0: nothing grabbed) */
    int32_t n_grabbed;               /* len(gripper.grabbed_pts) */
    int32_t iters_pull;
    int32_t n_below_half_thickness;  /* compute_height numerator (cloth_env.py:603-609) */
    uint8_t ran;                     /* 0: slot not executed (episode over and no reset script left) */
    uint8_t oob, tear, done;
    uint8_t reset_before;            /* k > 0: the env was reset right before this action, by its k-th script of this launch */
    uint8_t _pad[3];
} ClothStepRecord;

/* one consumed reset script */
typedef struct ClothResetRecord {
    int32_t consumed;                /* 0 no; 1 yes (complete record); 2 cut by the time slice, completed by the next launch */
    int32_t pulls_run;               /* scripted pulls executed (tier 1: 2 or 3) */
    int32_t executed[3];             /* update() calls of each pull */
    int32_t settle_executed;
    int32_t tear;                    /* Cloth.have_tear after the reset */
    int32_t init_side;               /* device-drawn resets: Cloth.init_side (cloth.pyx:75: np_random.rand() > 0.5) */
    double start_coverage, start_variance_inv;   /* cloth_env.py:780-782 */
    double action[3][4];             /* the reset actions in clip space, as the reference passes them to step(initialize=True) */
} ClothResetRecord;

/* T action slots for every env. policy: CLOTHHIP_POLICY_*. actions: [T][E][4] (TABLE), a HOST pointer unless
 * actions_on_device != 0 (a device table, e.g. after an RCCL broadcast). policy_arg: NULL, or how every cloth was built, int32[E]: 0 = the
 * flat tiers, 1 = tier 2 with init_side False (ORACLE_CORNER then swaps its corner indices, analytic.py:108-114), 2 = tier 2
 * with init_side True; a tier-2 reset inside the launch updates it. HIGHEST_POINT needs it and T more rows, int32[1 + T][E]:
 * row 1 + t = which of the highest points (0 = the highest) the env pulls in its t-th slot. scripts: [E][n_scripts] or NULL -- the
 * env's next resets in order. Script k+1 is drawn (by the host) from the RNG state script k leaves when only its
 * unconditional pulls run; if a conditional pull (tier 1's third, cloth_env.py:866) does run, it consumes further draws,
 * the later scripts of that env are void, and the env idles once its next episode ends (the host re-draws them for the
 * next launch). num_steps[E], done[E]: in/out episode state (ClothEnv.num_steps; episode over). records: [T][E].
 * resets: [E][n_scripts] or NULL. obs: [T][E][3P] float32 '1d' observation after each executed slot, or NULL. reset_obs:
 * [E][n_scripts][3P] float32 first observation of each episode started inside the launch (what env.reset() returns), or
 * NULL.
 * time_budget_ms > 0 makes the launch a TIME SLICE: an env starts no further action once the launch has run that long
 * (constant-rate 100 MHz clock), so envs advance at their own pace and the launch does not wait for the env with the most
 * work; the unused slots of an env stay `ran == 0` at the END of its column and the caller passes those actions again in
 * the next launch. The slice cuts operations in the middle (at a substep boundary): the handle keeps what is needed to
 * continue them, the next launch does so first, and the action's record appears in the launch that completes it (slot 0
 * of that env). A reset cut that way has consumed == 2 in this launch's record and its complete record (consumed == 1) in the
 * next one's slot 0; a slice may also end right after a reset (consumed == 1, no record with that reset_before). Any
 * other state-changing call on the handle (set_state, reset_flat, grab*, run*, update) drops the operations in flight.
 * Which launch executes an action never changes its result (envs are independent); only the partition
 * of an env's action sequence into launches depends on timing. 0 = every env executes all T slots.
 * The slice counts from each cloth's own start: a batch of more cloths than the device holds at once runs in generations,
 * each of them a kernel dispatch of its own on the handle's stream (the call is still one call, and
 * clothhip_last_kernel_ms spans all of them).
 * Returns CLOTHHIP_ESTATE when the handle's variant cannot run fused (per-env rest tables with reset scripts,
 * non-25x25 oracle policy, grid too large for the in-kernel metrics). Synchronous. */
/* Resets drawn ON THE DEVICE (the _begin/_end form only): instead of `scripts`, pass rng_states[E][626] = every env's
 * numpy RandomState (get_state(): key[624], pos, one pad word). The kernel then draws each reset exactly as ClothEnv.reset
 * does from np_random (cloth.pyx:75; cloth_env.py:851-877 tier 1 incl. the coverage-conditional third pull; :893-949 +
 * cloth.pyx:94-116 tier 2: the noisy vertical sheet, its rest lengths, 1500 + 500 settling updates, the two corner pulls --
 * the handle must hold per-env rest tables; :959-972 tier 3; rng_tier = 1, 2 or 3), bit for bit numpy's MT19937 / rand / uniform / randint stream (csrc/cloth_rng.hpp), skips
 * domrand_words 32-bit words after each reset (the domain-randomisation draws of cloth_env.py:786-789; 0 = none), and
 * _end returns the advanced states. n_scripts is then the capacity of resets[E][n_scripts] / reset_obs per env; any number
 * of resets per env and launch up to that capacity, no void scripts.
 * The same in two halves, so that the caller can work (e.g. draw the next reset scripts) while the launch runs:
 * _begin uploads the inputs and launches (the host input arrays are not retained), _end waits and downloads. The want_*
 * flags of _begin announce which of the optional output buffers _end will be given. One launch in flight per handle.
 * want_obs == 2 / want_reset_obs == 2: the table is written and kept on the device exactly as with 1, but not downloaded -- _end must be
 * given NULL for it (clothhip_render_obs and clothhip_fit_data_append_launch read it there). */
int clothhip_run_actions_begin(clothhip_handle *h, const ClothEpisodeParams *ep, int32_t T, int32_t policy,
                               const double *actions, int32_t actions_on_device, const int32_t *policy_arg,
                               const ClothResetScript *scripts, int32_t n_scripts, const int32_t *num_steps,
                               const uint8_t *done, const uint32_t *rng_states, int32_t rng_tier, uint64_t domrand_words,
                               int32_t want_resets, int32_t want_obs, int32_t want_reset_obs, double time_budget_ms);
int clothhip_run_actions_end(clothhip_handle *h, int32_t *num_steps, uint8_t *done, ClothStepRecord *records,
                             ClothResetRecord *resets, float *obs, float *reset_obs, uint32_t *rng_states);
/* Per-env summary of the last clothhip_run_actions launch, written by the kernel: summary[E][4] = {actions the env executed (slots with ran != 0),
 * 1 if its episode is over, the coverage after its last action or reset of the launch (NaN: it did neither), the Cloth.update()
 * calls of its actions}. `summary` (host, may be NULL) receives a copy; `d_summary` (may be NULL) receives the DEVICE address of the
 * table, valid for the handle's life and ordered on the handle's stream: the multi-GPU driver all-gathers it in place
 * (ncclAllGather) without staging through the host. Call after clothhip_run_actions_begin (the device address) or after _end (the
 * copy). No reference counterpart. */
int clothhip_run_actions_summary(clothhip_handle *h, double *summary, void **d_summary);
/* Where the time of the last clothhip_run_actions launch went, per env: ticks[E][8] = 100 MHz ticks (s_memrealtime) the env's
 * workgroup spent in {0: actions (ClothEnv.step incl. decode, grab_top, metrics), 1: scripted reset pulls (cloth_env.py:851-982) incl.
 * the coverage test of tier 1's third pull, 2: reset settling (bare update() calls), 3: the rest (Cloth() rebuild, idling once its
 * action slots are used up)}, then the Cloth.update() calls executed in each of the four classes. The benchmark derives the
 * action-only rate of SURVEY 8d from it. Call after clothhip_run_actions / _end. No reference counterpart. */
int clothhip_run_actions_op_ticks(clothhip_handle *h, uint64_t *ticks);
/* 1 if this handle's kernel variant has the LDS room for the in-kernel metrics of clothhip_run_actions, else 0 */
int clothhip_fused_supported(const clothhip_handle *h);

/* A learned policy inside the episode launch (no reference counterpart): a fully-connected network over the '1d' observation
 * (cloth_env.py:196-200), n_layers weight layers (1..4), widths[0 .. n_layers] with widths[0] = 3 P, widths[n_layers] = 4, hidden widths in
 * [1, 256], ReLU after every layer but the last (the launch's decode clips to act_low / act_high as for any action). params: ONE float32
 * blob of n_params values, for l = 0 .. n_layers-1 W_l[out][in] row-major (torch.nn.Linear.weight's layout), then b_l[out]. The input
 * is (float)position, element 3 i + ax, also on an fp64 handle, and the arithmetic is float32 in one fixed order
 * (csrc/cloth_policy_mlp.hpp), so the network is one function of the observation the caller would have seen, whatever stepper variant
 * runs. The call validates, uploads (the host blob is not retained) and replaces any earlier network; n_layers == 0 clears it.
 * CLOTHHIP_EINVAL: more than 4 layers, widths[0] != 3 P, a last width other than 4, a hidden width outside [1, 256], n_params not what
 * the widths give -- the earlier network then stays. This network belongs to the HANDLE: every env evaluates it (one network per env
 * slot: clothhip_set_policy_population below, which this call drops);
 * clothhip_fork, resets and clothhip_set_state never touch it. CLOTHHIP_ESTATE between clothhip_run_actions_begin and _end.
 * clothhip_run_actions* with CLOTHHIP_POLICY_MLP evaluates it once per action slot, when the slot begins (after an in-kernel reset: on the
 * new episode's first state), act = (double)y + actions[t][e] (`actions` optional there: the caller's exploration noise, NULL = none;
 * the record's `action` holds that sum before clipping); an action a time slice cuts is not evaluated again. CLOTHHIP_ESTATE from
 * those calls without a network, on a relaxed-order handle, or when the variant's LDS scratch cannot hold the two hidden vectors. */
int clothhip_set_policy_mlp(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, size_t n_params);
/* The handle's network on n float32 rows obs_rows[n][3P] (host), or with obs_rows == NULL on the handle's present state (n must then be
 * E): actions_out[n][4], the network's output as doubles, no noise, not clipped -- the very device function the launch runs, one
 * workgroup per row, the rows in bounded chunks. CLOTHHIP_ESTATE without a network or with a launch in flight. Synchronous. */
int clothhip_policy_eval(clothhip_handle *h, const float *obs_rows, int64_t n, double *actions_out);

/* A POPULATION of networks, one per env slot (no reference counterpart: what evolution strategies, CEM over parameters, population-based
 * training or ten checkpoints side by side need -- E cloths under E different networks in ONE episode launch). G blobs of one shape (the
 * shape rules of clothhip_set_policy_mlp), params[G][n_params] on the host; the handle stores them at a stride of n_params rounded up to 64
 * floats (every blob 256-byte aligned, the pad zeros) with the device table member[E], 0 <= member[e] < G: env slot e runs blob member[e].
 * A cloth under blob g computes the bits a handle with g as its shared network computes (only a base pointer moves). The network belongs
 * to the ENV SLOT, as the material does: uploads, clothhip_reset_flat, in-kernel resets and parked time-slice operations never touch it;
 * clothhip_fork carries no networks. The shared network and a population replace each other: setting one drops the
 * other; n_layers == 0 drops both. CLOTHHIP_EINVAL: the shape rules, G < 1, a member outside [0, G) -- the earlier network then stays (an
 * allocation or upload that fails leaves the handle without one). */
int clothhip_set_policy_population(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, int32_t G,
                                   const int32_t *member);
/* the map alone: member[E], each in [0, rows) (rows = G, or G + 1 after clothhip_policy_population_perturb). CLOTHHIP_ESTATE without a population. */
int clothhip_set_policy_members(clothhip_handle *h, const int32_t *member);
/* download blob g (g = 0 for a shared network): out[n_params], n_params what the handle's widths give -- or, for a population, the row stride
 * (n_params rounded up to 64), which gives the row's pad as well */
int clothhip_get_policy_mlp(clothhip_handle *h, int64_t g, float *out, size_t n_params);
/* clothhip_policy_eval with a network per row: row r is evaluated under blob members[r] (host int32 [n]); obs_rows == NULL: the handle's
 * present state, n == E. The same kernel in the same chunks. On a shared-network handle the only blob is 0. The plain clothhip_policy_eval
 * on a population handle is refused with CLOTHHIP_ESTATE: it cannot say which network a row means. */
int clothhip_policy_eval_members(clothhip_handle *h, const float *obs_rows, int64_t n, const int32_t *members, double *actions_out);

/* Make the population ON THE DEVICE (no reference counterpart; csrc/cloth_policy_population.hpp has the definition): G + 1 rows around the
 * blob center[n_params] = theta. With CLOTHHIP_POP_ANTITHETIC (G even) rows 2k and 2k + 1 are theta + sigma eps_k and theta - sigma eps_k,
 * without it row g is theta + sigma eps_g; row G is theta itself. eps_k[i] is a function of (seed, k, i) alone: Philox4x32-10 keyed by the
 * two halves of seed on the counter (i_lo, i_hi, k, 0), the four words' top 24 bits summed and centred, times (float)(sqrt(3) / 2^24) --
 * zero mean, unit variance, exactly symmetric, |eps| <= 3.47: the sum of four uniforms, NOT a Gaussian. A weight is
 * (float)((double)theta[i] + (double)(+-sigma) * (double)eps). member[E], each in [0, G]. The handle remembers (seed, sigma, flags, G, theta).
 * CLOTHHIP_EINVAL: the shape rules, G outside [1, 65534], odd G with the flag, unknown flags, a non-finite sigma, a member outside [0, G]
 * -- the earlier network then stays. clothhip_last_kernel_ms gives the kernel's time. */
enum { CLOTHHIP_POP_ANTITHETIC = 1 };
int clothhip_policy_population_perturb(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *center, int32_t G,
                                       float sigma, uint64_t seed, int32_t flags, const int32_t *member);
/* out[i] = (float) sum_{k ascending} (double)coef[k] * (double)eps_k[i], i < n_params, eps made again from the remembered seed: the
 * evolution-strategies update without a second copy of the noise. K = G / 2 with the antithetic flag, G without; anything else is
 * CLOTHHIP_EINVAL. CLOTHHIP_ESTATE without a population, or with one that was uploaded rather than generated. clothhip_last_kernel_ms
 * gives the kernel's time. The rows themselves are not read: after clothhip_policy_fit_members has trained them the sum is still that
 * of the last perturb's noise. */
int clothhip_policy_population_combine(clothhip_handle *h, const float *coef, int32_t K, float *out);

/* An EXPERT beside the acting policy (DAgger: examples/analytic.py's oracle says what it would have done in every state the learner
 * reached, and may take some of the actions over). clothhip_run_actions_expert arms the NEXT clothhip_run_actions / _begin on this handle,
 * and only that one: any such call consumes the arming, also one that fails. expert: CLOTHHIP_POLICY_ORACLE_CORNER or
 * CLOTHHIP_POLICY_HIGHEST_POINT. The armed launch evaluates the expert when a slot begins, where its acting policy is evaluated (after an
 * in-kernel reset: on the new episode's first state), on the same resident state and with the arithmetic a launch with that policy as its
 * acting policy performs -- policy_arg row 0 says how each cloth was built, exactly as for the acting policies; the highest-point k comes
 * from choice[t][e], not from policy_arg -- and writes labels[t][e][4]: what that launch would have put into ClothStepRecord.action,
 * unclipped, in clip space when clip_act_space is set. THE BITS: labels[t][e] of an armed launch == the `action` record of slot t of a
 * launch from the same state whose acting policy is the expert, as long as both executed the same actions before that slot (so always
 * for t = 0), and == clothhip_policy_label on the handle's state at that moment; on an fp32 handle also == clothhip_policy_label on the
 * float32 observation the slot's policy saw (on an fp64 handle that observation has rounded the positions, the label has not).
 * mix[T][E] (host, NULL = the expert never acts): mix[t][e] != 0 makes the label the slot's action -- act = label, no noise added, the
 * network not evaluated; otherwise the acting policy's action is taken as in an unarmed launch, whose records, states and observations an
 * armed launch with mix == 0 reproduces bit for bit. Only CLOTHHIP_POLICY_TABLE and CLOTHHIP_POLICY_MLP may act beside an expert.
 * choice[T][E] (host): HIGHEST_POINT only. Both tables are copied by this call. Time slices: an action a slice cuts is not planned
 * again and its label is not computed again; the label appears in the slot of its record, slot 0 of that env in the launch that
 * completes the action, provided that launch is armed too (the caller passes the unused mix / choice rows again, as for actions).
 * CLOTHHIP_EINVAL: an unknown expert, T < 1, HIGHEST_POINT without choice; at the armed _begin a T other than the armed one or an acting
 * policy other than TABLE / MLP. CLOTHHIP_ESTATE: arming with a launch in flight, a relaxed-order handle, a variant without the build
 * that carries the cold policies, ORACLE_CORNER on a grid other than 25x25. In all these cases nothing on the handle changes except that
 * the arming is gone. No reference counterpart. */
int clothhip_run_actions_expert(clothhip_handle *h, int32_t expert, int32_t T, const uint8_t *mix, const int32_t *choice);
/* After the armed launch (clothhip_run_actions_end or the synchronous form): labels[T][E][4], NaN where the slot's `ran` is 0. `labels` (host,
 * may be NULL) receives a copy, `d_labels` (may be NULL) the device address, as clothhip_run_actions_summary's d_summary. CLOTHHIP_ESTATE
 * with a launch in flight or when the last launch was not armed. */
int clothhip_run_actions_labels(clothhip_handle *h, double *labels, void **d_labels);
/* The expert on stored observations obs_rows[n][3P] (host float32, element 3 i + ax), or with obs_rows == NULL and n == E on the handle's
 * present state: actions_out[n][4] as above (clip_act_space: the launch's ClothEpisodeParams field). Positions go float -> double (the
 * state: handle precision -> double), from there the arithmetic is the launch's. side: int32[n] as policy_arg row 0 (0 flat tiers, 1 / 2
 * tier 2 with init_side False / True; NULL = all 0). choice: int32[n], HIGHEST_POINT only (clamped to [0, P - 1] as in the launch). One
 * 64-lane wave per row, the rows in bounded chunks as clothhip_policy_eval. CLOTHHIP_EINVAL: an unknown expert, n < 0, n != E with
 * obs_rows == NULL, HIGHEST_POINT without choice, actions_out == NULL with n > 0. CLOTHHIP_ESTATE: a launch in flight, ORACLE_CORNER on a
 * grid other than 25x25, HIGHEST_POINT on a grid whose row of heights exceeds 64 KiB of LDS (more than 16 384 points in float32). Synchronous; clothhip_last_kernel_ms gives the kernel's time (the last chunk's). Leaves an arming alone. */
int clothhip_policy_label(clothhip_handle *h, int32_t expert, int32_t clip_act_space, const float *obs_rows, int64_t n,
                          const int32_t *side, const int32_t *choice, double *actions_out);

/* FIT the handle's shared network ON THE DEVICE (no reference counterpart: the refit half of a DAgger / behaviour-cloning iteration):
 * a mean-squared-error fit of (observation row, action label) pairs that updates the float32 blob of clothhip_set_policy_mlp in place,
 * so the next episode launch runs the new weights with no download and no upload. csrc/cloth_policy_fit.hpp has the kernels and the
 * order of the arithmetic.
 * THE DATASET lives on the handle's device and survives across calls (DAgger's D <- D u D_i). clothhip_fit_data_append adds n pairs:
 * obs_rows[n][3P] (host float32, element 3 i + ax as clothhip_policy_eval reads it) and labels[n][4] (host doubles, stored as
 * (float)label). CLOTHHIP_EINVAL for n < 0, a NULL table with n > 0, or a non-finite observation or label (after the rounding to
 * float) -- nothing is appended then; the rows of slots that did not run carry NaN labels (clothhip_run_actions_labels), so the
 * caller passes the rows that ran. The storage grows geometrically. _clear empties it (the memory stays), _size reports the rows.
 * The dataset belongs to the handle: clothhip_fork does not carry it and clothhip_set_policy_* leave it alone. */
int clothhip_fit_data_append(clothhip_handle *h, const float *obs_rows, const double *labels, int64_t n);
int clothhip_fit_data_clear(clothhip_handle *h);
int clothhip_fit_data_size(clothhip_handle *h, int64_t *n);
/* Download stored rows [first, first + n): obs[n][3P] and labels[n][4], float32 as stored; either pointer may be NULL. For tests, and for
 * whoever checkpoints a dataset that grew without the host ever seeing it. CLOTHHIP_EINVAL for a range outside the dataset. */
int clothhip_fit_data_get(clothhip_handle *h, int64_t first, int64_t n, float *obs, float *labels);
/* PER-ROW LOSS WEIGHTS (fitting from reward: reward- or advantage-weighted regression, imitation of the best rollouts, and with
 * w_r = 2 A_r / sigma^2 the REINFORCE step of a fixed-sigma Gaussian policy, whose gradient the weighted MSE gradient then is). The
 * dataset has a third column w[n], float32, and the trainer's loss multiplies row r's squares by w_r (THE LOSS below). Every row
 * appended by clothhip_fit_data_append or clothhip_fit_data_append_launch gets 1.0f; the column grows with the rows and
 * clothhip_fit_data_clear empties it. The column is MUTABLE where the rows are not: a row has to be appended before the next launch
 * overwrites the observation it was taken on, while its return is known only when its episode ends, possibly several launches later
 * -- so the weight is written after the row. _set_weights writes w[0 .. n) to the stored rows [first, first + n), _get_weights reads
 * them. A weight is any finite float: negative and zero are allowed. CLOTHHIP_EINVAL for a range outside the dataset, a NULL table
 * with n > 0 or a non-finite weight -- nothing is written then; CLOTHHIP_ESTATE with a launch in flight. Synchronous.
 * clothhip_fit_data_append_weighted is clothhip_fit_data_append with weights[n] (NULL: 1.0f for every row) and its refusals, and a
 * non-finite weight refused as there. */
int clothhip_fit_data_set_weights(clothhip_handle *h, int64_t first, int64_t n, const float *w);
int clothhip_fit_data_get_weights(clothhip_handle *h, int64_t first, int64_t n, float *w);
int clothhip_fit_data_append_weighted(clothhip_handle *h, const float *obs_rows, const double *labels, const float *weights, int64_t n);
/* ROWS NAMED BY WHERE THEY LIE ON THE DEVICE (csrc/cloth_fit_gather.hpp): a DAgger collection appends what each slot's policy saw without
 * the observation tables ever leaving the device. A row is (source, row):
 *   CLOTHHIP_FIT_SRC_SLOTS   row t * E + e of the last launch's observation table (the state after slot t of env e);
 *   CLOTHHIP_FIT_SRC_RESETS  row e * n_scripts + k of its reset-observation table (the first state of env e's k-th episode of the launch);
 *   CLOTHHIP_FIT_SRC_HELD    row e of held[E][3P] float32, a table of the handle that outlives the launch tables.
 * The launch tables are valid as for clothhip_render_obs: from the _end of a launch that was given want_obs / want_reset_obs (1, or 2 =
 * kept on the device and not downloaded) until the next clothhip_run_actions* call on the handle, which overwrites them -- also one that
 * fails after its argument checks: the tables are then gone and these calls refuse them; no other call touches
 * them (clothhip_set_state, clothhip_fork, resets and the fit leave them alone -- they describe the launch, not the present state).
 * The label table is that of the last launch and exists only if that launch was armed (clothhip_run_actions_expert).
 * clothhip_fit_hold fills held: with src == NULL, held[e] = the float32 '1d' observation of env e's PRESENT state (the arithmetic of
 * clothhip_write_obs_f32_device); else src[E][2] = (source, row) and held[e] = the named row, where (CLOTHHIP_FIT_SRC_HELD, e) for env e
 * keeps the row it has (another env's held row cannot be named). The copy has completed when the call returns, so the next launch may
 * overwrite the launch tables.
 * clothhip_fit_data_append_launch appends n pairs in the order given, rows[n][3] = (source, row, label_row): the observation is the named
 * row, the label (float)labels[label_row][0..3] of the last armed launch's table (label_row = t * E + e; the rounding of
 * clothhip_fit_data_append). The storage grows as there. The kernel writes into the spare capacity behind the stored rows and raises a
 * flag when an observation value or a rounded label is not finite (the label of a slot that did not run is NaN): the rows count only if
 * the flag stayed clear, else CLOTHHIP_EINVAL with clothhip_fit_data_append's message for the first such value (entry and element) and
 * the dataset is what it was. Synchronous; clothhip_last_kernel_ms gives the kernel's time.
 * Refused before anything is touched -- CLOTHHIP_ESTATE: a launch in flight, SLOTS / RESETS when the last launch kept no such table (or
 * there was none), a label row when the last launch was not armed, HELD before any clothhip_fit_hold; CLOTHHIP_EINVAL: an unknown source,
 * a row outside its table, n < 0, rows == NULL with n > 0, more than INT32_MAX rows in all.
 * clothhip_fit_data_append_launch_ex is that call with a LABEL SOURCE and the rows' weights (weights[n] in entry order, host, any finite
 * float, NULL: 1.0f); clothhip_fit_data_append_launch(h, rows, n) IS _ex(h, rows, n, CLOTHHIP_FIT_LABEL_EXPERT, NULL).
 *   CLOTHHIP_FIT_LABEL_EXPERT  the label table of the last armed launch, as above;
 *   CLOTHHIP_FIT_LABEL_ACTION  label_row = t * E + e names the last launch's ClothStepRecord ON THE DEVICE and the label is
 *        (float)record.action[0..3]: what step() was passed, before clipping -- for CLOTHHIP_POLICY_MLP the network's output plus the
 *        caller's noise, the sample the launch EXECUTED. No armed expert is needed. The record table is valid under the rule of the
 *        observation tables: from a launch's _end (or the synchronous form) until the next clothhip_run_actions* call. A named record
 *        with ran != 1 is the NaN label of a slot that did not run: the flag is raised, CLOTHHIP_EINVAL, the dataset is what it was.
 * The refusals are those above; besides, CLOTHHIP_ESTATE for LABEL_ACTION with no launch since creation (or none whose record table
 * is still there), CLOTHHIP_EINVAL for an unknown label_src or a non-finite weight. */
enum { CLOTHHIP_FIT_SRC_SLOTS = 0, CLOTHHIP_FIT_SRC_RESETS = 1, CLOTHHIP_FIT_SRC_HELD = 2 };
enum { CLOTHHIP_FIT_LABEL_EXPERT = 0, CLOTHHIP_FIT_LABEL_ACTION = 1, CLOTHHIP_FIT_LABEL_ZERO = 3 /* ACTOR-CRITIC below; 2 names no source and stays refused */,
       CLOTHHIP_FIT_LABEL_ACTION_EXPERT = 4 /* DDPG FROM DEMONSTRATIONS below */ };
int clothhip_fit_hold(clothhip_handle *h, const int32_t *src);
int clothhip_fit_data_append_launch(clothhip_handle *h, const int32_t *rows, int64_t n);
int clothhip_fit_data_append_launch_ex(clothhip_handle *h, const int32_t *rows, int64_t n, int32_t label_src, const float *weights);
/* THE LOSS over a minibatch of B dataset rows idx[0 .. B) (host int32, repeats allowed and counted as often), with y the network's
 * float32 output, a the stored label and w_r the stored weight of row r:   L = 1 / (4 B) sum_r w_r sum_k (y_rk - a_rk)^2   (with every
 * weight 1: torch.nn.MSELoss()), so dL/dy_rk = w_r (y_rk - a_rk) / (2 B). The normaliser is B, not sum w: the caller normalises the
 * weights. The arithmetic: dz_rk = fl(fl(w_r fl(y - a)) / fl(2 B)) in float32; the loss adds (double)w_r * (dd * dd) with
 * dd = (double)y - (double)a, each operation one double rounding, thread t of 256 taking elements t, t + 256, ... of the [B][4] table
 * in ascending order, the 256 sums added by a halving tree, the total divided by 4 B. Multiplying by 1.0f and by 1.0 is exact, so a
 * dataset whose weights are all 1 -- every dataset that no weight was written to -- gives the bits of the unweighted loss.
 * ReLU's derivative is 1 where the pre-activation is > 0, else 0. clothhip_policy_fit_grad computes L (a double: the squares are summed
 * in double in a fixed order) and dL/dtheta (grad_out[n_params] float32, the blob's layout) at the handle's present weights and updates
 * nothing. All arithmetic is float32, on an fp64 handle too, on the f32-input matrix instructions; every reduction has one fixed order
 * and there are no floating-point atomics, so two runs give the same bits. The trainer's forward sums in another order than
 * clothhip_policy_eval, so its y need not equal that function's bits. */
int clothhip_policy_fit_grad(clothhip_handle *h, const int32_t *idx, int32_t B, float *grad_out, double *loss_out);
/* THE LOSS ALONE over any number n >= 1 of dataset rows idx[0 .. n) (a held-out split by index), forward only, nothing updated:
 * L = 1 / (4 n) sum_r w_r sum_k (y_rk - a_rk)^2, weighted as above. The rows go through the trainer's forward in chunks of at most CLOTHHIP_FIT_MAX_BATCH, in
 * order; a chunk's squares are summed as clothhip_policy_fit_grad sums them, the chunk sums are added in ascending order in double, and
 * the total is divided once by 4 n -- so for n <= CLOTHHIP_FIT_MAX_BATCH the result is clothhip_policy_fit_grad's loss bit for bit.
 * The refusals of clothhip_policy_fit_grad, with n in place of B and no upper limit but INT32_MAX. */
int clothhip_policy_fit_loss(clothhip_handle *h, const int32_t *idx, int64_t n, double *loss);
/* THE TRAINER'S FORWARD on stored rows named by index, nothing updated: y_out[r][0..3] (host float32 [n][4]) is bit for bit the y that
 * clothhip_policy_fit_grad forms for row idx[r] (which clothhip_policy_eval's need not be: another summation order). It lets the host
 * compute weights from the network's own outputs on rows it never downloaded: residuals, trust-region masks, an ensemble's
 * disagreement on the dataset. Any n >= 1, in chunks of at most CLOTHHIP_FIT_MAX_BATCH (an output row depends on its own row alone,
 * so the chunking shows nowhere). clothhip_policy_fit_predict: the shared network, the refusals of clothhip_policy_fit_loss.
 * clothhip_policy_fit_predict_members: y_out[n_m][n][4], the SAME rows idx[n] for every member, the refusals of the _members calls
 * (the cap on n_m * B applies to a chunk: n_m <= CLOTHHIP_FIT_MAX_MEMBER_ROWS, and the chunks shorten to fit). */
int clothhip_policy_fit_predict(clothhip_handle *h, const int32_t *idx, int64_t n, float *y_out);
int clothhip_policy_fit_predict_members(clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int64_t n, float *y_out);
/* The optimizer. All fields are floats; lr, eps, momentum finite and >= 0, beta1 and beta2 in [0, 1).
 *   CLOTHHIP_FIT_ADAM  with t the 1-based count of steps since the last reset, the host computes in double
 *        a_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)  and hands the device (float)a_t, (float)(1 - beta1), (float)(1 - beta2); per parameter,
 *        every fl one float32 operation (no contraction; division and square root correctly rounded):
 *        m = fl(fl(beta1 m) + fl((1 - beta1) g));  v = fl(fl(beta2 v) + fl((1 - beta2) fl(g g)));
 *        theta = fl(theta - fl(a_t fl(m / fl(sqrtf(v) + eps))))
 *   CLOTHHIP_FIT_SGD   u = fl(fl(momentum u) + g);  theta = fl(theta - fl(lr u))
 * No weight decay. The per-row weights are the dataset's (PER-ROW LOSS WEIGHTS above), not the optimizer's. SGD's u and Adam's m are
 * ONE table: change the optimizer through clothhip_policy_fit_reset. */
enum { CLOTHHIP_FIT_ADAM = 0, CLOTHHIP_FIT_SGD = 1 };
typedef struct ClothFitParams { float optimizer /* CLOTHHIP_FIT_* */, lr, beta1, beta2, eps, momentum; } ClothFitParams;
/* n_steps optimizer steps; step s uses the rows idx[s][0 .. B) (host int32 [n_steps][B]: which rows a step uses is the caller's table)
 * and loss_out[s] (may be NULL) is the loss BEFORE that step's update. The gradient inside a step is bit for bit what
 * clothhip_policy_fit_grad returns for the same weights and rows (the same kernels). The moments and the step count persist across
 * calls; clothhip_policy_fit_reset zeroes them, and so do clothhip_set_policy_mlp and clothhip_set_policy_population. Synchronous;
 * clothhip_last_kernel_ms gives the time of all n_steps steps on the device.
 * CLOTHHIP_ESTATE (both calls): no shared network on the handle, a population on it (the fit trains the ONE shared network), a launch
 * in flight, an empty dataset. CLOTHHIP_EINVAL: B < 1 or B > CLOTHHIP_FIT_MAX_BATCH (the activations of one step: at most 4 hidden and
 * 2 gradient tables of B x 256 floats and the split batch sums of the weight gradients, some 60 MB at the cap), n_steps < 0, an index
 * outside [0, dataset size), an unknown optimizer, a non-finite or negative hyper-parameter or a beta outside [0, 1), a NULL table.
 * A refused call changes nothing: not the network, not the moments, not the step count. */
#define CLOTHHIP_FIT_MAX_BATCH 4096
int clothhip_policy_fit(clothhip_handle *h, const ClothFitParams *p, const int32_t *idx, int32_t n_steps, int32_t B, double *loss_out);
int clothhip_policy_fit_reset(clothhip_handle *h);
/* FIT ROWS OF A POPULATION in the launches of one network (no reference counterpart: a bootstrapped ensemble for DAgger, a learning-rate
 * sweep, population-based training). members[n_m] (host int32) are DISTINCT rows of the handle's population (clothhip_set_policy_population
 * or clothhip_policy_population_perturb, whose centre row may be named too), in any order, a subset or all. The dataset is the handle's
 * one dataset; member j has its own minibatches: idx[n_steps][n_m][B] (for the gradient idx[n_m][B]) -- the bootstrap -- and its own
 * hyper-parameters p[j] (p[n_m]; the `optimizer` fields of one call must all be equal). Row members[j] is updated in place where it
 * lies, so the next episode launch with CLOTHHIP_POLICY_MLP, clothhip_policy_eval_members and clothhip_get_policy_mlp see the new weights
 * with no upload. Rows not named keep their bytes, and no call writes the pad floats of a row (n_params .. stride).
 * THE BITS. After any sequence of these calls, row g and its optimizer state are what a second handle holds that was given g as its
 * shared network (clothhip_set_policy_mlp), stores the same dataset and received the same sequence of
 * clothhip_policy_fit(p[j], idx[:, j, :]) calls: there is one trainer, whose kernels carry the member as one more grid index (the
 * shared network is its call members = {0}, n_m = 1), and no output element depends on it (csrc/cloth_policy_fit.hpp). So EVERY ROW has its own Adam
 * m, v (SGD u) and its own 1-based step count t: a row trained in two calls of 2 steps equals one trained in one call of 4, and a row
 * that joins later starts at t = 1. a_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) is made in double on the host per member and step, as for
 * clothhip_policy_fit, and goes up as one table per call. clothhip_policy_fit_grad_members returns for member j the gradient
 * (grad_out[j][n_params], may be NULL) and the loss (loss_out[j], may be NULL) that clothhip_policy_fit_grad returns on that handle and
 * updates nothing. clothhip_policy_fit_members: loss_out[s][j] (may be NULL) is member j's loss BEFORE step s. All n_steps are enqueued
 * behind one upload of the tables; synchronous; clothhip_last_kernel_ms gives the time of all steps on the device.
 * THE OPTIMIZER STATE lives with the population: clothhip_set_policy_mlp, clothhip_set_policy_population and
 * clothhip_policy_population_perturb restart every row (the rule of the shared trainer); clothhip_set_policy_members (the map alone)
 * restarts nothing; clothhip_policy_fit_reset_members restarts the rows named (members == NULL: all rows; n_m is then ignored).
 * clothhip_policy_population_combine is untouched by a fit: it sums the noise of the last perturb from its seed, whatever the rows hold now.
 * SCRATCH is sized on demand: per member the activations, two dZ tables, the gradient and (B > 256) the split batch sums, hence the
 * cap on n_m * B.
 * Refused before anything is touched -- CLOTHHIP_ESTATE: a launch in flight, no network, a shared network (use clothhip_policy_fit), an
 * empty dataset (not for the reset). CLOTHHIP_EINVAL: n_m < 1, a member outside [0, rows), a member named twice, B outside
 * [1, CLOTHHIP_FIT_MAX_BATCH], n_m * B > CLOTHHIP_FIT_MAX_MEMBER_ROWS, n_steps < 0, an index outside the dataset, a hyper-parameter
 * clothhip_policy_fit would refuse, differing optimizer fields, NULL where a table is needed. n_steps == 0 returns 0 and changes
 * nothing. clothhip_policy_fit, _fit_grad, _fit_loss and _fit_reset keep refusing a population. */
#define CLOTHHIP_FIT_MAX_MEMBER_ROWS 65536   /* n_m * B of one call */
int clothhip_policy_fit_grad_members(clothhip_handle *h, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B, float *grad_out,
                                     double *loss_out);
int clothhip_policy_fit_members(clothhip_handle *h, const ClothFitParams *p, const int32_t *members, int32_t n_m, const int32_t *idx,
                                int32_t n_steps, int32_t B, double *loss_out);
int clothhip_policy_fit_reset_members(clothhip_handle *h, const int32_t *members, int32_t n_m);

/* ACTOR-CRITIC FROM REWARD (no reference counterpart): a VALUE NETWORK V(s) over the stored observation rows, fitted to
 * value targets by the one trainer, and generalised advantage estimation written into the dataset's weight column on the device.
 * THE VALUE NETWORK. clothhip_set_value_mlp takes the shape rules and the blob layout of clothhip_set_policy_mlp, except that
 * widths[n_layers] == 1. It belongs to the handle, beside the policy and independent of it: setting or dropping a policy network or a
 * population leaves it (and its optimizer state) alone, and the reverse; n_layers == 0 drops it; a refused call keeps the earlier one;
 * clothhip_fork does not carry it; no episode launch evaluates it. clothhip_get_value_mlp downloads the blob (out[n_params]).
 * CLOTHHIP_ESTATE with a launch in flight, and from _get without a value network.
 * EPISODE STRUCTURE AND VALUE TARGETS are three more columns of the dataset beside the weights; they grow with the rows and
 * clothhip_fit_data_clear empties them:
 *   rew[n]  float32  the reward of the action executed from the row's state. Default 0.
 *   next[n] int32    the dataset index of the row that holds the successor state of the same episode; or
 *                    CLOTHHIP_FIT_NEXT_TERMINAL: the episode ended there, the successor's value is 0; or CLOTHHIP_FIT_NEXT_NONE (the
 *                    default): the row is a LEAF -- it has no transition of its own and serves only as a successor whose value bootstraps.
 *   ret[n]  float32  the value target. Default 0.
 * clothhip_fit_data_set_transitions writes rew and next of the rows [first, first + n), _set_returns writes ret; the _get calls download
 * them. A successor index must be STRICTLY GREATER than the row's own index and below the dataset's size (rows are appended in time
 * order, so a successor lies later: every chain is finite and acyclic without a check on the device). Refused, nothing written --
 * CLOTHHIP_EINVAL: a range outside the dataset, a value that is not finite, a next that is none of the three, a NULL table with n > 0;
 * CLOTHHIP_ESTATE: a launch in flight.
 * CLOTHHIP_FIT_LABEL_ZERO is a third label source of clothhip_fit_data_append_launch_ex: the label is (0, 0, 0, 0), label_row is
 * ignored, and neither an armed expert nor a record that ran is needed -- how a leaf is appended from where it lies on the device.
 * FITTING THE CRITIC. The value network is one more one-row weight table of the trainer above (the same kernels, its own moments, its
 * own step count, the same lazy reset):  L_V = 1 / (2 B) sum_r (v_r - ret_r)^2, UNWEIGHTED (the weight column belongs to the policy),
 * dz_r = fl(fl(v_r - ret_r) / fl(B)); the loss adds dd * dd, dd = (double)v - (double)ret, in the order of clothhip_policy_fit_grad
 * (thread t of 256 takes rows t, t + 256, ..., then the halving tree) and divides by 2 B. clothhip_value_fit_grad, clothhip_value_fit
 * and clothhip_value_fit_reset are clothhip_policy_fit_grad, clothhip_policy_fit and clothhip_policy_fit_reset for it, with their
 * refusals and "no value network" in place of "no shared network"; a population on the handle is no obstacle (the critic is not the
 * policy). clothhip_value_predict: v_out[n] float32 for any n >= 1 stored rows, in chunks of at most CLOTHHIP_FIT_MAX_BATCH, bit for
 * bit the v of clothhip_value_fit_grad. No critic call changes a bit of the policy's blob, moments or step count, and the reverse.
 * ADVANTAGES AND VALUE TARGETS ON THE DEVICE. clothhip_fit_data_gae runs the critic's forward over the rows [first, first + n) (the
 * launches of clothhip_value_predict, the values stay on the device), then for a NON-LEAF row r walks the chain r_0 = r,
 * r_k+1 = next[r_k], which stops after a row whose next is TERMINAL or whose successor is a leaf. Every operation is one double rounding:
 *   nv = (double)v[next] (0 when next is TERMINAL);  delta = ((double)rew + gamma nv) - (double)v;
 *   A = 0, coef = 1; for k ascending: A = A + coef delta_k, then coef = coef c, with c = gamma lambda formed once in double on the host;
 *   adv_r = (float)A;  ret[r] <- (float)(A + (double)v_r).
 * A LEAF row: adv = 0, ret <- v of the leaf. With CLOTHHIP_GAE_WRITE_WEIGHTS the weight column of the range is written too:
 * w[r] <- (float)((double)w_scale A^), 0 for a leaf, where A^ = A, or with CLOTHHIP_GAE_NORMALIZE A^ = (A - mean) / (std + 1e-8), mean and
 * population standard deviation over the non-leaf rows of the range, in double, in two passes (the sum of A, then the sum of
 * (A - mean)^2, each divided by the count), each pass in the order above: thread t of 256 takes rows t, t + 256, ... of the range, then
 * the halving tree. Without CLOTHHIP_GAE_WRITE_WEIGHTS the weight column is untouched. adv_out[n] and ret_out[n] (host float32) may be
 * NULL. No floating-point atomics: two runs give the same bits. Synchronous; clothhip_last_kernel_ms gives the forward and the scan.
 * Refused before anything is touched -- CLOTHHIP_ESTATE: no value network, a launch in flight; CLOTHHIP_EINVAL: a range outside the
 * dataset, gamma, lambda or w_scale not finite, gamma or lambda outside [0, 1], unknown flags, p == NULL, a row of the range whose
 * successor lies outside the range. n == 0 returns 0. */
enum { CLOTHHIP_FIT_NEXT_TERMINAL = -1, CLOTHHIP_FIT_NEXT_NONE = -2 };
enum { CLOTHHIP_GAE_WRITE_WEIGHTS = 1, CLOTHHIP_GAE_NORMALIZE = 2 };
typedef struct ClothGaeParams { double gamma, lambda; float w_scale; int32_t flags /* CLOTHHIP_GAE_* */; } ClothGaeParams;
int clothhip_set_value_mlp(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, size_t n_params);
int clothhip_get_value_mlp(clothhip_handle *h, float *out, size_t n_params);
int clothhip_fit_data_set_transitions(clothhip_handle *h, int64_t first, int64_t n, const float *rew, const int32_t *next);
int clothhip_fit_data_get_transitions(clothhip_handle *h, int64_t first, int64_t n, float *rew, int32_t *next);
int clothhip_fit_data_set_returns(clothhip_handle *h, int64_t first, int64_t n, const float *ret);
int clothhip_fit_data_get_returns(clothhip_handle *h, int64_t first, int64_t n, float *ret);
int clothhip_value_fit_grad(clothhip_handle *h, const int32_t *idx, int32_t B, float *grad_out, double *loss_out);
int clothhip_value_fit(clothhip_handle *h, const ClothFitParams *p, const int32_t *idx, int32_t n_steps, int32_t B, double *loss_out);
int clothhip_value_fit_reset(clothhip_handle *h);
int clothhip_value_predict(clothhip_handle *h, const int32_t *idx, int64_t n, float *v_out);
int clothhip_fit_data_gae(clothhip_handle *h, int64_t first, int64_t n, const ClothGaeParams *p, float *adv_out, float *ret_out);

/* PPO ON THE DEVICE (no reference counterpart): the clipped surrogate of a Gaussian policy with a fixed standard
 * deviation sigma and the shared network's output as its mean, over stored OLD MEANS. A weighted squared error under a negative weight
 * has no minimum, so a collection paid for one policy-gradient step; the clipped surrogate switches a row's gradient off once its
 * probability ratio has left [1 - eps, 1 + eps] in the direction its advantage pushes, so many steps on one collection stay bounded.
 * The advantages are the dataset's weight column (clothhip_fit_data_gae with w_scale 1 writes them), the actions its labels.
 * THE OLD MEANS are a fifth column of the dataset, old[n][4] float32: what the policy's mean was when the row was collected. It grows
 * with the rows, keeps its contents on growth and clothhip_fit_data_clear empties it. A row appended by any entry has NO old mean
 * until one is written (the handle keeps one byte per row). clothhip_fit_data_snapshot_policy runs the trainer's forward of the shared
 * network over the rows [first, first + n) -- the launches of clothhip_policy_fit_predict, in chunks of at most
 * CLOTHHIP_FIT_MAX_BATCH -- and stores y into the column where it lies: nothing is downloaded, and the stored bytes are those
 * clothhip_policy_fit_predict returns for these rows. Its refusals are clothhip_policy_fit_predict's (CLOTHHIP_ESTATE: a launch in
 * flight, no shared network, a population on the handle -- clothhip_fit_data_snapshot_policy_members below is its snapshot --, an empty dataset) and CLOTHHIP_EINVAL
 * for a range outside the dataset; n == 0 returns 0. clothhip_fit_data_set_old_means writes mu[n][4] (host float32) to the rows and
 * marks them, _get_old_means downloads the column (zeros for a row without an old mean); both are refused as
 * clothhip_fit_data_set_returns is: a range outside the dataset, a value that is not finite, a NULL table with n > 0, a launch in flight.
 * THE LOSS over a minibatch of B rows, with mu = y the network's float32 output, a the stored label, mo the stored old mean and A the
 * stored weight of the row. The host forms in double, once: inv_s2 = 1 / (sigma sigma), half_inv_s2 = 0.5 inv_s2, lo = 1 - clip,
 * hi = 1 + clip. Per row, every operation ONE double rounding on the (double) of the float32 values, no contraction:
 *   q = 0; for k = 0 .. 3: q = q + (((a_k - mo_k) (a_k - mo_k)) - ((a_k - mu_k) (a_k - mu_k)))
 *   x = q half_inv_s2;  rho = exp_fixed(x)            the probability ratio pi(a) / pi_old(a); exp_fixed clamps x to [-40, 40] first
 *   s1 = rho A;  s2 = min(max(rho, lo), hi) A;  active = s1 <= s2           (inside the interval s1 == s2: active)
 *   dz_k = active ? (float)((((s1 (mu_k - a_k)) inv_s2) / (double)B) : 0.0f       = d(-s1 / B) / d mu_k
 *   surrogate = active ? s1 : s2  (= min(s1, s2));   kl = 0; for k = 0 .. 3: kl = kl + (mu_k - mo_k) (mu_k - mo_k);  kl_row = kl half_inv_s2
 * exp_fixed(x): x clamped to [-40, 40]; k = rint(x log2e); r = (x - k ln2_hi) - k ln2_lo with fdlibm's log2e = 1.44269504088896338700e+00,
 * ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10; p = 1 / 13!, then p = p r + 1 / i! for i = 12 .. 0 (a
 * product and a sum, each rounded; 1 / i! the correctly rounded quotient); the result p 2^k, exact. No library exp is called:
 * policies.exp_fixed_reference restates it in numpy bit for bit, and clothhip_selftest_exp_fixed runs the same function on the host
 * (out[i] = exp_fixed(x[i]); CLOTHHIP_EINVAL for a NaN). It is within 2.2e-16 relative of exp, and exp_fixed(0) == 1.0.
 * Three sums over the minibatch in the order of clothhip_policy_fit_grad's loss, over ROWS: thread t of 256 adds its rows t, t + 256,
 * ... ascending, the 256 sums are added by a halving tree. stats[0] = loss = -(sum surrogate) / B; stats[1] = clip_fraction = (rows
 * not active) / B; stats[2] = kl = (sum kl_row) / B. A caller stops its epochs on the last two. Everything behind dz is the
 * trainer's backward pass, unchanged; no floating-point atomics. With mo == mu and A = w sigma^2 / 2 the gradient is that of the
 * weighted squared error.
 * clothhip_policy_fit_ppo_grad is clothhip_policy_fit_grad for this loss: grad_out[n_params] (may be NULL), stats_out[3] (may be
 * NULL), ratio_out[B] (may be NULL) = (float)rho per minibatch row; nothing is updated. clothhip_policy_fit_ppo is
 * clothhip_policy_fit for it: stats_out[n_steps][3] (may be NULL) are each step's statistics BEFORE its update. It uses the POLICY'S
 * optimizer: a squared-error step and a PPO step of one handle share the moments and the step count, and clothhip_policy_fit_reset
 * restarts both. Refused before the first launch, nothing changed -- everything clothhip_policy_fit refuses (with q == NULL as a NULL
 * table); CLOTHHIP_EINVAL: sigma not finite or <= 0 (or so small that 1 / sigma^2 is not finite), clip not finite, < 0 or >= 1;
 * CLOTHHIP_ESTATE: an idx entry whose row has no old mean (the message names the row). Shared network only. */
typedef struct ClothPpoParams { double sigma, clip; } ClothPpoParams;
#define CLOTHHIP_PPO_STATS 3      /* loss, clip_fraction, kl */
int clothhip_fit_data_snapshot_policy(clothhip_handle *h, int64_t first, int64_t n);
int clothhip_fit_data_set_old_means(clothhip_handle *h, int64_t first, int64_t n, const float *mu);
int clothhip_fit_data_get_old_means(clothhip_handle *h, int64_t first, int64_t n, float *mu);
int clothhip_policy_fit_ppo_grad(clothhip_handle *h, const ClothPpoParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out, float *ratio_out);
int clothhip_policy_fit_ppo(clothhip_handle *h, const ClothFitParams *p, const ClothPpoParams *q, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out);

/* PPO WITH A LEARNED SIGMA (additive, ABI 7; no reference counterpart): the policy above with a state-independent
 * log sigma per action component that the same surrogate trains, and an entropy bonus that keeps it from collapsing. Every entry
 * above keeps its bytes; a handle that never calls an entry below behaves as before.
 * THE HEAD is log_sigma[4] float32 on the handle, beside the shared network's blob and not in it (the blob layout, n_params and
 * clothhip_get_policy_mlp are unchanged). clothhip_set_policy_log_sigma sets it (ls == NULL drops it) and restarts the head's
 * optimizer state, and that alone; CLOTHHIP_EINVAL for a value that is not finite or |ls_k| > 10, CLOTHHIP_ESTATE with a launch in
 * flight. clothhip_get_policy_log_sigma downloads it (CLOTHHIP_ESTATE without a head). Setting or dropping a network or a population
 * leaves the head's values alone; clothhip_fork and snapshots do not carry it (they carry no network either). NO EPISODE LAUNCH READS
 * IT: the action stays y + noise[t][e], and the caller scales unit noise by exp(log_sigma) on the host -- or lets
 * clothhip_policy_noise_fill (EXPLORATION NOISE ON THE DEVICE below) make the table from the head where it lies.
 * THE OLD LOG SIGMA is a sixth column of the dataset, old_ls[n][4] float32, default zeros, with its own byte per row on the handle: a
 * row appended by any entry has none. On a handle WITH a head clothhip_fit_data_snapshot_policy also writes the present head into the
 * rows of its range (a fill on the device, nothing downloaded) and marks them; without a head it does exactly what it did.
 * clothhip_fit_data_set_old_log_sigma / _get_old_log_sigma are the host route, refused as clothhip_fit_data_set_old_means is.
 * THE LOSS over a minibatch of B rows: ls the head, lo the row's old log sigma, mu = y, mo, a, A as above; lo_c = 1 - clip,
 * hi_c = 1 + clip formed once in double on the host. Every operation ONE double rounding on the (double) of the float32 values, no
 * contraction; the only exponential is exp_fixed. Once per launch: inv_k = exp_fixed(-2 ls_k). Per row:
 *   for k = 0 .. 3: invo_k = exp_fixed(-2 lo_k);  so2_k = exp_fixed(2 lo_k);
 *     t_old = ((a_k - mo_k) (a_k - mo_k)) invo_k;  t_new_k = ((a_k - mu_k) (a_k - mu_k)) inv_k;
 *     q = q + (((t_old - t_new_k) 0.5) + (lo_k - ls_k))                                   (q = 0 before k = 0)
 *     klq = klq + (((so2_k inv_k) - 1) + (((mu_k - mo_k) (mu_k - mo_k)) inv_k));  kld = kld + (ls_k - lo_k)      (both 0 before k = 0)
 *   kl_row = kld + (klq 0.5)            KL(old || new) of the two diagonal Gaussians
 *   rho = exp_fixed(q);  s1 = rho A;  s2 = min(max(rho, lo_c), hi_c) A;  active = s1 <= s2
 *   dz_k = active ? (float)((((s1 (mu_k - a_k)) inv_k) / (double)B) : 0.0f
 *   h_k = active ? s1 (t_new_k - 1) : 0            the row's term of d(s1) / d ls_k
 *   surrogate = active ? s1 : s2
 * Seven sums over the rows in the order above (thread t of 256 its rows t, t + 256, ... ascending, then a halving tree each): the
 * surrogate, the rows not active, kl_row and the four h_k. With hs = ((ls_0 + ls_1) + ls_2) + ls_3 (from 0) the entropy is
 * H = hs + 5.675754132818691 (= 2 (1 + ln 2 pi)), and
 *   stats[0] = (-(sum surrogate) / B) - (ent_coef H);  stats[1] = (rows not active) / B;  stats[2] = (sum kl_row) / B;  stats[3] = H;
 *   grad_ls_k = (float)((-(sum h_k) / B) - ent_coef).
 * With ls == lo == 0 (exp_fixed(0) == 1.0, products by 1.0 and 0.5 are exact, a sum of halves is half the sum) a row's rho, dz, the
 * surrogate and -- with ent_coef 0 -- the first three statistics are the bytes clothhip_policy_fit_ppo_grad gives at sigma = 1.
 * Outside [-20, 20] the clamp inside exp_fixed (its argument to [-40, 40]) defines the arithmetic; the optimizer does not clamp the head.
 * THE ENTRIES. clothhip_policy_fit_ppo_sigma_grad: grad_out[n_params], grad_ls_out[4], stats_out[4], ratio_out[B], each may be
 * NULL; nothing is updated. clothhip_policy_fit_ppo_sigma: n_steps steps; stats_out[n_steps][4] and log_sigma_out[n_steps][4] (both
 * may be NULL) are the statistics and the head BEFORE each step's update. Forward, backward, the blob's optimizer, its moments and step
 * count are clothhip_policy_fit_ppo's. The head is updated by the SAME optimizer kernel, launched a second time over a table of one row
 * of four elements, under the call's ClothFitParams, with its own moments and its own 1-based step count (a_t formed in double on the
 * host from that count). clothhip_policy_fit_reset restarts the head's optimizer state too; clothhip_set_policy_log_sigma restarts
 * it alone. Refused before the first launch, nothing changed -- everything clothhip_policy_fit_ppo refuses (a population among it);
 * CLOTHHIP_ESTATE: no head on the handle, an idx entry whose row has no old mean or no old log sigma (the message names the row);
 * CLOTHHIP_EINVAL: clip not finite, < 0 or >= 1, ent_coef not finite or < 0. */
typedef struct ClothPpoSigmaParams { double clip, ent_coef; } ClothPpoSigmaParams;
#define CLOTHHIP_PPO_SIGMA_STATS 4      /* loss, clip_fraction, kl, entropy */
int clothhip_set_policy_log_sigma(clothhip_handle *h, const float *ls);
int clothhip_get_policy_log_sigma(clothhip_handle *h, float *out);
int clothhip_fit_data_set_old_log_sigma(clothhip_handle *h, int64_t first, int64_t n, const float *ls);
int clothhip_fit_data_get_old_log_sigma(clothhip_handle *h, int64_t first, int64_t n, float *ls);
int clothhip_policy_fit_ppo_sigma_grad(clothhip_handle *h, const ClothPpoSigmaParams *q, const int32_t *idx, int32_t B, float *grad_out, float *grad_ls_out, double *stats_out, float *ratio_out);
int clothhip_policy_fit_ppo_sigma(clothhip_handle *h, const ClothFitParams *p, const ClothPpoSigmaParams *q, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out, float *log_sigma_out);

/* PPO FOR A POPULATION (additive, ABI 7; no reference counterpart): PPO ON THE DEVICE for rows of a population, every
 * member under its own sigma, clip range and optimizer, all members in the launches of one network -- a sweep over learning rate,
 * sigma, clip and seed at the cost of one configuration's collection and one grouped fit. Every entry above keeps its bytes and its
 * refusals (the shared-network entries still refuse a population); a handle that never calls an entry below behaves as before.
 * THE OLD MEAN OF A ROW is the mean of its BEHAVIOUR policy: of the member that ran the env the row was collected from. The ratio
 * pi_new / pi_behaviour is defined for any learner, so the dataset's ONE old-mean column serves every member; there is no column per
 * member and nothing records which member owns a row.
 * clothhip_fit_data_snapshot_policy_members: member_of_row[n] (host int32) names for every row of [first, first + n) a population
 * row g >= 0 -- row first + i then gets the trainer's forward of row g on it, the bytes
 * clothhip_policy_fit_predict_members({g}, 1, {first + i}, 1) returns, and is marked as having an old mean -- or -1: the row is
 * skipped, its bytes and its mark stay. Nothing is downloaded. The host groups the rows by member (members without rows take no part),
 * cuts a member's list into segments of at most CLOTHHIP_FIT_MAX_BATCH rows and launches the forward of
 * clothhip_policy_fit_grad_members over as many segments as CLOTHHIP_FIT_MAX_MEMBER_ROWS holds, shorter segments padded with a row of
 * their own; one more kernel scatters each member's y to its rows of the column, a 16-byte store per row, nothing for a padded
 * position. With a log-sigma head on the handle the old-log-sigma column is NOT touched. Refused before the first launch, nothing
 * changed -- CLOTHHIP_ESTATE: a launch in flight, no network, a shared network, an empty dataset; CLOTHHIP_EINVAL: a range outside the
 * dataset, member_of_row == NULL with n > 0, an entry < -1 or >= the population's rows (the message names its position). n == 0 or
 * all entries -1 returns 0.
 * THE LOSS is PPO ON THE DEVICE's, operation by operation, with member j's own q[j] = {sigma, clip}: the host forms inv_s2,
 * half_inv_s2, lo, hi of every member in double by the expressions above, and they go up as one table [n_m][4] of which member j's
 * workgroup reads row j (the shared network's entries send a table of one row to the same kernel). clothhip_policy_fit_ppo_grad_members is clothhip_policy_fit_grad_members for it: grad_out[n_m][n_params],
 * stats_out[n_m][3], ratio_out[n_m][B], each may be NULL; nothing is updated. clothhip_policy_fit_ppo_members is
 * clothhip_policy_fit_members for it: idx[n_steps][n_m][B], stats_out[n_steps][n_m][3] (may be NULL) each member's statistics BEFORE
 * each step. They use the population's per-row optimizer state: a squared-error group step and a PPO group step of one row share its
 * moments and its step count, and clothhip_policy_fit_reset_members restarts both.
 * THE BITS are the twin's, as for FIT ROWS OF A POPULATION: after any sequence of calls, row g, its moments and its step count are
 * what a second handle holds that carries g as its shared network, stores the same dataset, weights and old means and received
 * clothhip_policy_fit_ppo(p[j], q[j], idx[:, j, :]).
 * Refused before the first launch, nothing changed -- everything clothhip_policy_fit_members refuses; CLOTHHIP_EINVAL: q == NULL,
 * sigma_j or clip_j outside clothhip_policy_fit_ppo's domain (the message names j); CLOTHHIP_ESTATE: an idx entry whose row has no
 * old mean (the message names the row and the member). n_steps == 0 returns 0.
 * OUT OF SCOPE: per-member log-sigma heads, per-member critics, a clipped value loss, per-member normalisation of the advantages on
 * the device (the host normalises: demos.ppo_fit), noise drawn inside the launch. */
int clothhip_fit_data_snapshot_policy_members(clothhip_handle *h, int64_t first, int64_t n, const int32_t *member_of_row /* [n] */);
int clothhip_policy_fit_ppo_grad_members(clothhip_handle *h, const ClothPpoParams *q, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t B, float *grad_out, double *stats_out, float *ratio_out);
int clothhip_policy_fit_ppo_members(clothhip_handle *h, const ClothFitParams *p, const ClothPpoParams *q, const int32_t *members, int32_t n_m, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out);

/* EXPLORATION NOISE ON THE DEVICE (additive, ABI 7; no reference counterpart): the table double [T][E][4] that an episode
 * launch under CLOTHHIP_POLICY_MLP adds to the network's output, made on the handle's device by one fill kernel
 * (csrc/cloth_policy_noise.hpp) and handed to clothhip_run_actions_begin as its device-resident table (actions_on_device = 1). Every
 * entry above keeps its bytes; no stepper kernel and no launch record changes; a handle that never calls an entry below behaves as
 * before.
 * THE KEY. noise[t][e][k] = sigma[e][k] z_k(seed, e, slot_base[e] + t), ONE double multiplication; z depends on (seed, env, that env's
 * slot number) and nothing else -- not T, not E, not the launch, not how a collection is cut into launches.
 * THE VARIATE z[0..3] = normal_fixed(seed, e, s) (csrc/cloth_philox.hpp; references.normal_fixed_reference restates it bit for bit): four
 * independent standard normals by Box-Muller, every operation ONE IEEE double rounding, no contraction, no library log / sin / cos;
 * division and sqrt are the correctly rounded ones. For pair j = 0, 1:
 *   r[0..3] = Philox4x32-10(counter = ((uint32)s, (uint32)(s >> 32), e, 0x4E000000 + j), key = ((uint32)seed, (uint32)(seed >> 32)))
 *            (the tag in the fourth word keeps these counters apart from population_eps', whose fourth word is 0)
 *   n1 = ((uint64)r[0] << 20) | (r[1] >> 12);  u1 = ((double)n1 + 0.5) 2^-52                      exact, in (0, 1)
 *   n2 = ((uint64)r[2] << 20) | (r[3] >> 12);  q = n2 >> 50;  t = (((double)(n2 mod 2^50) + 0.5) 2^-50) - 0.5      exact, in (-1/2, 1/2)
 *   x = t * 1.5707963267948966;  x2 = x x
 *   C = Horner in x2 over (-1)^i / (2 i)!, i = 10 .. 0;  S = Horner in x2 over (-1)^i / (2 i + 1)!, i = 10 .. 0 (p = (p x2) + c_i each);
 *   c = C;  s = x S;  (c, s) <- (c, s), (-s, c), (-c, -s), (s, -c) for q = 0 .. 3
 *   log_fixed(u1): u1 = m 2^k from its bits, m in [1, 2);  if m >= 1.4142135623730951: m = m 0.5, k = k + 1;
 *     f = m - 1;  g = m + 1;  v = f / g;  w = v v;  P = Horner in w over 1 / (2 i + 1), i = 13 .. 0;
 *     L = (((2 v) P) + ((double)k ln2_lo)) + ((double)k ln2_hi)          (exp_fixed's two fdlibm constants)
 *   rad = sqrt(-2 L);  z[2 j] = rad c;  z[2 j + 1] = rad s
 * |z| reaches 8.57. Every constant is a correctly rounded quotient of exact integers, pi / 2 or a half of ln 2.
 * clothhip_policy_noise_fill fills the handle's table for T slots on the handle's stream -- the launch that follows is ordered behind
 * it without a synchronisation -- and returns where it lies in *d_noise (may be NULL); the table belongs to the handle and stays
 * valid until the next fill or clothhip_destroy. slot_base[E] (host, may be NULL: zeros) numbers row t of env e as slot
 * slot_base[e] + t. sigma (host) is [4] for all envs with sigma_rows = 1, or [E][4] with sigma_rows = E; sigma == NULL with
 * sigma_rows = 0 takes the handle's log-sigma head: every thread reads log_sigma[4] where it lies and forms
 * exp_fixed((double)log_sigma[k]) -- the sigma that acts is bit for bit the one PPO WITH A LEARNED SIGMA differentiates, and nothing is
 * downloaded. One thread per (t, e), workgroups of 256, two 16-byte stores per thread; clothhip_last_kernel_ms times it.
 * Refused, nothing changed -- CLOTHHIP_ESTATE: a clothhip_run_actions_begin in flight (that launch may be reading the table), no head
 * on the handle when the head is asked for; CLOTHHIP_EINVAL: T < 1 or T E > 2^31 - 1, sigma_rows not 1 or E with a table (not 0
 * without one), a sigma that is not finite or negative, a negative slot_base (or one whose slot_base + T leaves 63 bits).
 * clothhip_policy_noise_get downloads the table of the last fill into out[T][E][4], for tests and for callers that want the host
 * array: CLOTHHIP_ESTATE before any fill or with a launch in flight, CLOTHHIP_EINVAL for a T other than the last fill's.
 * OUT OF SCOPE: drawing inside the stepper kernel, a state-dependent sigma, replacing population_eps in the population and the planner. */
int clothhip_policy_noise_fill(clothhip_handle *h, uint64_t seed, int32_t T, const int64_t *slot_base, const double *sigma, int32_t sigma_rows, void **d_noise);
int clothhip_policy_noise_get(clothhip_handle *h, int32_t T, double *out);

/* DDPG ON THE DEVICE (additive, ABI 7; the off-policy loop of the reference's cfg/demo_baselines*.yaml, no kernel counterpart there;
 * DESIGN 4.3.14): a Q CRITIC over (state, action), TARGET copies of the policy and of the critic with a soft update, the TD target read
 * through a row's successor, and the deterministic policy gradient -- the actor's dZ taken from the critic's input gradient. The
 * dataset is the replay buffer: a row's label is the action it executed (CLOTHHIP_FIT_LABEL_ACTION), rew and next are its transition,
 * and old collections stay in it. Every entry above keeps its bytes; a handle that never calls an entry below behaves as before.
 * THE Q NETWORK. clothhip_set_q_mlp takes the shape rules and the blob layout of clothhip_set_value_mlp, except widths[0] == 3 P + 4: a
 * row of its input is the '1d' observation followed by the four action components; widths[n_layers] == 1. It is independent of the
 * policy, the value network and the log-sigma head, and the reverse; n_layers == 0 drops it; a refused call keeps the earlier one;
 * clothhip_fork does not carry it; no launch evaluates it. It has its own optimizer state (moments, 1-based step count, the lazy reset
 * of the other tables), restarted by a new Q network and by clothhip_q_fit_reset. clothhip_get_q_mlp downloads the blob.
 * THE TARGETS are a second policy blob and a second Q blob on the handle. clothhip_ddpg_sync_targets copies the present shared policy
 * network and Q network into them, device to device; clothhip_ddpg_get_targets downloads them (either pointer may be NULL;
 * policy_out[the policy's n_params], q_out[the Q network's n_params]); clothhip_ddpg_set_targets uploads them, as a checkpoint restores
 * them (a NULL pointer leaves that target as it is; a blob has the layout and the size of the network it shadows, which must be there). A new policy network (or a population, or dropping it)
 * invalidates the target policy, a new Q network the target Q; entries that read or move a target then return CLOTHHIP_ESTATE until the
 * next sync. DDPG trains the ONE shared network: with a population on the handle every entry below returns CLOTHHIP_ESTATE.
 * THE CRITIC'S INPUT. k_fit_concat writes X[r][0 .. 3P) = obs[idx[r]][.], X[r][3P .. 3P + 4) = min(max(a_r, -bound), +bound) with
 * bound = act_bound (float32; +inf: no clamp; min and max are exact) and a_r the row's label (the critic's step) or a network's
 * float32 output (the target policy on the successor; the policy in the actor's step). The Q network's products run over X with the
 * kernels and the summation order of the value network's.
 * THE CRITIC'S STEP over a minibatch idx[B]. The host makes succ[r] = next[idx[r]] from its mirror of the next column (a TERMINAL
 * row: the row itself, whose value is ignored) and uploads it beside idx. mu' = target policy on obs[succ]; qn = target Q on
 * [obs[succ], clamp(mu')]; q = Q on [obs[idx], clamp(label)]. Per row, every operation ONE double rounding:
 *   nv = (double)qn_r, or 0 where next[idx[r]] is TERMINAL;  y_r = (float)((double)rew + (gamma nv))
 * then in float32 dz_r = fl(fl(q_r - y_r) / fl(B)); the loss adds dd dd, dd = (double)q - (double)y, in the order of
 * clothhip_value_fit_grad (thread t of 256 takes rows t, t + 256, ..., then the halving tree) and divides by 2 B.
 *   stats = {loss, (sum q) / B, (sum y) / B}        (CLOTHHIP_Q_STATS)
 * Everything behind dz is the trainer's backward pass. clothhip_q_fit_grad: grad_out[n_params of Q], stats_out[3], y_out[B],
 * q_out[B], each may be NULL; nothing is updated. clothhip_q_fit: n_steps optimizer steps under p over idx[n_steps][B],
 * stats_out[n_steps][3] (may be NULL) BEFORE each update. Neither moves a target.
 * THE ACTOR'S STEP minimises L = -1/B sum_r Q(s_r, clamp(mu(s_r))) over the policy's weights, the critic held fixed: mu = policy on
 * obs[idx]; Q's forward on [obs[idx], clamp(mu)]; the dZ of Q's last layer is the constant fl(-1.0f / fl(B)); Q's input gradients run
 * down to layer 0 (the masked product of the trainer's backward), and layer 0's is formed for the four action columns alone:
 * dA[B][4] = dZ_0 W_0[:, 3P .. 3P + 4), one accumulator per element, k ascending. No Q weight gradient is formed. The clamp's gate:
 *   dz_rk = 0 where (mu_rk >= bound and dA_rk < 0) or (mu_rk <= -bound and dA_rk > 0), else dA_rk
 * -- a component outside the box whose descent step would push it further out is held; inward moves pass.
 *   stats = {-(sum q) / B, gated / (4 B), (sum |dA_rk|) / (4 B)}      (CLOTHHIP_DPG_STATS; sums in double, rows in the order above, k ascending)
 * Everything behind dz is the trainer's backward pass of the policy. clothhip_policy_fit_dpg_grad: grad_out[n_params of the policy],
 * stats_out[3], da_out[B][4] = dA, each may be NULL; nothing is updated. clothhip_policy_fit_dpg: n_steps steps under p with the
 * POLICY'S optimizer state (shared with clothhip_policy_fit and clothhip_policy_fit_ppo; clothhip_policy_fit_reset restarts it);
 * stats_out[n_steps][3]. It reads no target.
 * THE SOFT UPDATE. clothhip_ddpg_polyak: target_i = fl(fl(omt target_i) + fl(t theta_i)) for both targets, t = (float)tau and
 * omt = (float)(1 - tau) formed in double on the host.
 * clothhip_ddpg_fit runs n_steps times: the critic's step under p_q, the actor's step under p_policy against the UPDATED critic, the
 * soft update of both targets by q->tau -- all enqueued behind one upload, synchronous; stats_out[n_steps][6] (may be NULL): the
 * critic's three, then the actor's three. It equals, by bytes, the same steps made of clothhip_q_fit (1 step),
 * clothhip_policy_fit_dpg (1 step) and clothhip_ddpg_polyak: the same launches in the same order. The Q passes have scratch tables of
 * their own, so the policy's activations survive them. No floating-point atomics anywhere: two runs give the same bits.
 * Refused before anything is touched, no network, target, moment or step count changed -- CLOTHHIP_ESTATE: a launch in flight, no
 * policy network, a population, no Q network, no valid target where the entry reads or moves one (clothhip_q_fit*, clothhip_ddpg_fit,
 * clothhip_ddpg_polyak), an empty dataset (not for sync, polyak and reset); CLOTHHIP_EINVAL: B outside [1, CLOTHHIP_FIT_MAX_BATCH],
 * n_steps < 0, an index outside the dataset, a LEAF row in idx (its next is CLOTHHIP_FIT_NEXT_NONE: it has no transition), gamma or tau
 * not finite or outside [0, 1], act_bound <= 0 or NaN, flags != 0, an optimizer clothhip_policy_fit would refuse, a NULL table.
 * n_steps == 0 returns 0.
 * clothhip_ddpg_last_tables (for tests of the elementwise kernels; nothing is computed) downloads what the LAST DDPG call of minibatches
 * of B rows left in the Q passes' scratch, each pointer may be NULL: x_out[B][3P + 4], the critic's input rows its last k_fit_concat
 * wrote; q_out[B], the critic's output of its last forward; qn_out[B], the target critic's values -- there only when the call ran a
 * critic's step (not after clothhip_policy_fit_dpg*), else CLOTHHIP_ESTATE. CLOTHHIP_ESTATE before any DDPG call on the present Q network,
 * CLOTHHIP_EINVAL for another B.
 * OUT OF SCOPE: twin critics, target smoothing, a delayed actor; DDPG for a population; prioritised replay, n-step targets; a tanh
 * output; reading the dataset as a second operand of the product in the place of the copy X. */
typedef struct ClothDdpgParams { double gamma, tau; float act_bound; int32_t flags /* none defined: 0 */; } ClothDdpgParams;
#define CLOTHHIP_Q_STATS 3        /* loss, mean q, mean y */
#define CLOTHHIP_DPG_STATS 3      /* loss = -mean q, gated fraction, mean |dL/da| */
#define CLOTHHIP_DDPG_STATS 6     /* clothhip_ddpg_fit: the critic's, then the actor's */
int clothhip_set_q_mlp(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, size_t n_params);
int clothhip_get_q_mlp(clothhip_handle *h, float *out, size_t n_params);
int clothhip_ddpg_sync_targets(clothhip_handle *h);
int clothhip_ddpg_get_targets(clothhip_handle *h, float *policy_out, float *q_out);
int clothhip_ddpg_set_targets(clothhip_handle *h, const float *policy, const float *q);
int clothhip_q_fit_grad(clothhip_handle *h, const ClothDdpgParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out, float *y_out, float *q_out);
int clothhip_q_fit(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out);
int clothhip_q_fit_reset(clothhip_handle *h);
int clothhip_policy_fit_dpg_grad(clothhip_handle *h, const ClothDdpgParams *q, const int32_t *idx, int32_t B, float *grad_out, double *stats_out, float *da_out);
int clothhip_policy_fit_dpg(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out);
int clothhip_ddpg_polyak(clothhip_handle *h, double tau);
int clothhip_ddpg_last_tables(clothhip_handle *h, int32_t B, float *x_out, float *qn_out, float *q_out);
int clothhip_ddpg_fit(clothhip_handle *h, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams *q, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out);

/* DDPG FROM DEMONSTRATIONS (additive, ABI 7; the actor loss of Nair et al., "Overcoming Exploration in Reinforcement
 * Learning with Demonstrations"): the deterministic policy gradient plus a behaviour-cloning term on the rows that carry an EXPERT
 * ACTION, under the Q-FILTER only where the critic rates the expert's action above the policy's own. Any row the learner reached can
 * carry one -- the expert armed beside the acting policy labels every state --, so these are DAgger's labels inside DDPG's loss. Every
 * entry above keeps its kernels, its launches and its bytes.
 * THE EXPERT COLUMN. A dataset row has one more column, float [4], whose default is four times the 32-bit pattern 0x7fc00000 (a quiet
 * NaN): "no expert action". A row has an expert action iff component 0 is not a NaN, tested on the bits:
 * (bits & 0x7fffffff) > 0x7f800000 means none; every writer stores four finite values or four fill patterns. Rows appended by any
 * earlier entry or label source read back as the fill. clothhip_fit_data_set_expert(h, first, n, a[n][4]): a row of four finite values
 * sets the expert action, a row of four NaNs (any NaNs) clears it and is stored as the fill; a row that mixes the two, or an infinity,
 * is CLOTHHIP_EINVAL and the dataset stays what it was. clothhip_fit_data_get_expert reads the column. Both refuse what
 * clothhip_fit_data_set_weights refuses.
 * CLOTHHIP_FIT_LABEL_ACTION_EXPERT is a fourth label source of clothhip_fit_data_append_launch_ex: the label is
 * (float)record.action[0..3] exactly as under LABEL_ACTION and the expert column gets (float)labels[label_row][0..3] of the last armed
 * launch exactly as the label does under LABEL_EXPERT, in the one kernel launch. It refuses what either source refuses:
 * CLOTHHIP_ESTATE for a launch that was not armed or no record table; CLOTHHIP_EINVAL, the dataset what it was, for a record with
 * ran != 1 or a rounded value of either that is not finite.
 * THE ACTOR'S STEP under ClothBcParams {q_coef, bc_coef, flags, reserved}, filter = flags & CLOTHHIP_BC_QFILTER. With the filter, first
 * k_fit_concat's expert mode writes X_E[r] = [obs[idx[r]], min(max(a_E, -bound), bound)] -- a row without an expert action gets four
 * 0.0f, by a select on the bit test -- and the live critic's forward over X_E gives qe[B] (computed and ignored on such a row), in the
 * activation slot the critic's step uses for the target critic. Then the sequence of clothhip_policy_fit_dpg up to dA, and
 * k_fit_dpg_bc in the place of the gate. Per minibatch row r: m_r = the row has an expert action; f_r = m_r and (no filter or
 * qe_r > q_r), the comparison strict and in float32 (a tie does not pass). Per component k, every operation ONE float32 rounding:
 *   g = the gate above (0 where held, else dA_rk);  a = fl(q_coef g)
 *   where f_r and bc_coef != 0:  e = min(max(a_E_rk, -bound), bound);  d = fl(y_rk - e);  b = fl(fl(bc_coef d) / fl(2 B));  dz_rk = fl(a + b)
 *   elsewhere dz_rk = a, and NO addition is made: the sign of a zero survives, and with q_coef = 1 (an exact product) dz is
 *   clothhip_policy_fit_dpg's by bytes.
 * No gradient flows through the filter or through e. The BC loss adds dd dd, dd = (double)y_rk - (double)e, over the rows with f_r
 * (thread t of 256 takes rows t, t + 256, ..., k ascending, then the halving tree) and is reported over 4 B, NOT scaled by bc_coef: the
 * normalisation of clothhip_policy_fit's loss, B and not the number of labelled rows -- the caller scales bc_coef.
 *   stats = {-(sum q) / B, gated / (4 B), (sum |dA|) / (4 B), bc_loss, (sum m_r) / B, (sum f_r) / B}     (CLOTHHIP_DPG_BC_STATS; the first three are CLOTHHIP_DPG_STATS)
 * With q_coef = 0, bc_coef = 1, no filter and every row labelled the gradient EQUALS clothhip_policy_fit_grad's on labels
 * clamp(a_E) with weights 1 as numbers, not by bytes: 0 g may be -0, and x + (-0) differs from x only in the sign of a zero.
 * clothhip_policy_fit_dpg_bc_grad: grad_out[n_params of the policy], stats_out[6], da_out[B][4], dz_out[B][4], q_out[B], qe_out[B],
 * each may be NULL; qe_out without the filter is CLOTHHIP_EINVAL; nothing is updated. clothhip_policy_fit_dpg_bc: n_steps steps under
 * p with the policy's optimizer state, stats_out[n_steps][6]. clothhip_ddpg_fit_bc: clothhip_ddpg_fit with this actor's step,
 * stats_out[n_steps][9] (the critic's three, then these six); it equals, by bytes, clothhip_q_fit (1 step),
 * clothhip_policy_fit_dpg_bc (1 step) and clothhip_ddpg_polyak one call at a time. Without the filter no extra concat or forward is
 * launched. A minibatch with no labelled row is legal: a DPG step scaled by q_coef. None of the three changes the Q network (but
 * clothhip_ddpg_fit_bc's critic step), the value network, the head or a dataset column.
 * Refused before anything is touched: what the DDPG entries refuse, and CLOTHHIP_EINVAL for a coefficient that is NaN, infinite or
 * negative, both coefficients 0, unknown flags, reserved != 0.
 * After a call of these with the filter, clothhip_ddpg_last_tables' x_out is X_E (the expert rows have a table of their own) and its
 * qn_out is refused as after an actor's step: that slot holds qe.
 * OUT OF SCOPE: TD3, n-step targets, prioritised replay, BC for a population, a BC term in the critic. */
typedef struct ClothBcParams { float q_coef, bc_coef; int32_t flags; int32_t reserved; } ClothBcParams;
#define CLOTHHIP_BC_QFILTER 1
#define CLOTHHIP_DPG_BC_STATS 6   /* CLOTHHIP_DPG_STATS, then bc_loss, labelled share, filter-pass share */
#define CLOTHHIP_DDPG_BC_STATS 9  /* clothhip_ddpg_fit_bc: the critic's, then the BC actor's */
int clothhip_fit_data_set_expert(clothhip_handle *h, int64_t first, int64_t n, const float *a);
int clothhip_fit_data_get_expert(clothhip_handle *h, int64_t first, int64_t n, float *a);
int clothhip_policy_fit_dpg_bc_grad(clothhip_handle *h, const ClothDdpgParams *q, const ClothBcParams *bc, const int32_t *idx, int32_t B, float *grad_out, double *stats_out, float *da_out, float *dz_out, float *q_out, float *qe_out);
int clothhip_policy_fit_dpg_bc(clothhip_handle *h, const ClothFitParams *p, const ClothDdpgParams *q, const ClothBcParams *bc, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out);
int clothhip_ddpg_fit_bc(clothhip_handle *h, const ClothFitParams *p_policy, const ClothFitParams *p_q, const ClothDdpgParams *q, const ClothBcParams *bc, const int32_t *idx, int32_t n_steps, int32_t B, double *stats_out);

int clothhip_run_actions(clothhip_handle *h, const ClothEpisodeParams *ep, int32_t T, int32_t policy,
                         const double *actions, int32_t actions_on_device, const int32_t *policy_arg,
                         const ClothResetScript *scripts, int32_t n_scripts, int32_t *num_steps, uint8_t *done,
                         ClothStepRecord *records, ClothResetRecord *resets, float *obs, float *reset_obs,
                         double time_budget_ms);

/* ---- PLAN ACTIONS ON THE DEVICE: the cross-entropy method over forked cloths, the simulator itself as the model (no reference counterpart;
 * gym-cloth's follow-up work plans with CEM over a learned model). csrc/cloth_plan.hpp has the two kernels.
 * NAMES. E = envs of the SOURCE handle `src`, K = candidates per env, H = horizon in actions, M = elites, it = iteration in [0, n_iters). The
 * SCRATCH handle has exactly E K cloths on src's device, in its precision, grid and ClothParams (the caller creates it); branch (e, k) lives
 * in its slot e K + k. All planner arithmetic is float64 on both precisions (action tables are doubles), one operation per fl(), no
 * contraction. mean[E][H][4] and std[E][H][4] are in/out. done[e] != 0 marks env e as NOT PLANNED: its mean / std rows stay untouched, its
 * best_actions rows and best_score are NaN; its branches are forked and launched like the others (a done env executes nothing) and ignored.
 * SAMPLE (k_plan_sample).  x[h][e K + k][a] = clip(fl(mean[e][h][a] + fl(std[e][h][a] * (double)eps)), act_low[a], act_high[a]) with
 *   eps = population_eps(seed, iter0 + it, ((e K + k) H + h) 4 + a) -- the exact variate of clothhip_policy_population_perturb (Philox4x32-10 keyed
 *   by seed on the counter (index lo, index hi, iter0 + it, 0); zero mean, unit variance, |eps| <= 3.47) --, clip(v, lo, hi) = v < lo ? lo :
 *   (v > hi ? hi : v), act_low / act_high those of ClothEpisodeParams. Candidate k = 0 is clip(mean) itself, without noise. The table has
 *   clothhip_run_actions' [T = H][E K][4] layout and is written into the device buffer the launch reads.
 * ROLL OUT.  One clothhip_fork: src env e -> scratch slots e K .. e K + K - 1, materials included. Then ONE episode launch on the scratch handle:
 *   CLOTHHIP_POLICY_TABLE, T = H, actions_on_device, no reset scripts, no time budget, num_steps[e] and done[e] of the source replicated K times
 *   -- so max_actions, a tear or leaving the bounds end a branch where they would end the episode.
 * SCORE.  Branch (e, k) is scored on the device from its record column: its executed slots are those with ran != 0;
 *   score = coverage of the last executed slot, minus `penalty` when any executed slot has oob or tear; a branch without an executed slot scores
 *   -infinity (a branch of a planned env whose episode has actions left always executes slot 0).
 * ELITES.  rank_k = #{j : score_j > score_k or (score_j == score_k and j < k)}: candidates ordered by (score descending, k ascending), a counting
 *   rank, so equal scores have one defined order. The M candidates of rank < M are the elites, the one of rank 0 is the top candidate.
 * REFIT (k_plan_refit: one workgroup per env, its scores in LDS).  For each (h, a) one thread loops over the elites in ascending k, x the clipped
 *   table values:  mu = (sum x_k) / M;  var = (sum (x_k - mu)^2) / M;  sd = sqrt(var) (division and square root correctly rounded);
 *   mean <- fl(fl(alpha mu) + fl(beta mean));  std <- max(min_std[a], fl(fl(alpha sd) + fl(beta std)));  beta = 1 - alpha, made once on the host.
 * BEST SO FAR.  The iteration's top candidate replaces best_actions[e][H][4] / best_score[e] only if its score is strictly greater than
 *   best_score[e]; iteration 0 always sets them. So best_score[e] is the running maximum of the top scores.
 * BOUNDS.  horizon in [1, 8], n_candidates in [2, 1024], n_elite in [1, n_candidates], n_iters >= 1, iter0 + n_iters <= 2^31, alpha in (0, 1],
 *   penalty finite, min_std finite and >= 0, std finite and >= 0, mean finite. */
typedef struct ClothPlanParams {
    int32_t horizon, n_candidates, n_elite, n_iters;
    uint64_t seed;
    uint32_t iter0;
    int32_t _pad;
    double alpha, penalty;
    double min_std[4];
} ClothPlanParams;
/* The whole loop, n_iters x { sample, fork, launch, score + refit }, in one call. ep, num_steps[E], done[E] as clothhip_run_actions takes them
 * for the source (read only). mean / std [E][H][4]: in the initial distribution, out the last refit's. best_actions[E][H][4], best_score[E].
 * scores_out[n_iters][E][K] and cands_out[n_iters][H][E K][4] (the clipped tables) are optional (NULL), for tests and diagnostics; they are
 * gathered on the device and downloaded with the results after the last iteration. The launch's records are scored where they lie (the
 * planner ends the launch through a library-internal path instead of clothhip_run_actions_end, which would download them): between
 * iterations nothing comes back from the device, and what goes up is what clothhip_fork (its index lists) and clothhip_run_actions_begin
 * (the replicated counters and flags, the argument block) upload on every call.
 * CLOTHHIP_EINVAL: anything outside the bounds, a NULL table, bad episode parameters, scratch == src, a scratch handle of another size,
 * precision, grid, device or ClothParams. CLOTHHIP_ESTATE: a clothhip_run_actions_begin in flight on either handle, a parked time-slice
 * operation on a planned source env (clothhip_in_flight), a scratch handle that cannot run fused (clothhip_fused_supported), a relaxed-order
 * scratch handle. A refused call changes nothing; the source handle's state is never written. Synchronous; the scratch handle's cloths, its
 * last-launch tables and clothhip_last_kernel_ms (the last iteration's launch) are the planner's afterwards. */
int clothhip_plan_cem(clothhip_handle *scratch, clothhip_handle *src, const ClothEpisodeParams *ep, const ClothPlanParams *params,
                      const int32_t *num_steps, const uint8_t *done, double *mean, double *std, double *best_actions, double *best_score,
                      double *scores_out, double *cands_out);
/* The two kernels alone, on host tables and without a cloth (h gives the device and the stream only; E >= 1 is the caller's).
 * _sample: iteration `it` of params (iter = iter0 + it; n_elite, n_iters, alpha, penalty, min_std are not read): mean, std [E][H][4] ->
 *   x_out[H][E K][4].
 * _refit: the action table x[H][E K][4] and a score table scores[E][K] (no NaN; +-infinity allowed) -> mean, std (in/out), elite[E][K] (1 for
 *   an elite, else 0; all 0 for an env that is not planned) and top[E] (the top candidate's k, -1 for an env that is not planned). done[E] or
 *   NULL = every env planned. elite and top may be NULL.
 * The bounds and CLOTHHIP_EINVAL as above; CLOTHHIP_ESTATE with a launch in flight on h. */
int clothhip_plan_sample(clothhip_handle *h, const ClothPlanParams *params, const double act_low[4], const double act_high[4], int32_t E,
                         int32_t it, const double *mean, const double *std, double *x_out);
int clothhip_plan_refit(clothhip_handle *h, const ClothPlanParams *params, int32_t E, const double *x, const double *scores,
                        const uint8_t *done, double *mean, double *std, uint8_t *elite, int32_t *top);

/* Convenience: n x Cloth.update() on every env (cloth_env.py:902-903, :948-949, :980-981), optionally
 * preceded each time by Gripper.adjust(delta) when delta != NULL ([3] doubles, same for all envs). */
int clothhip_update(clothhip_handle *h, int32_t n_sub, const double *delta);

/* Per-env quantities ClothEnv derives from the particle positions after every action:
 *   coverage[E]      area of the 2-D convex hull of (clip(x,0,1), clip(y,0,1))  (cloth_env.py:628-638, :1086-1098;
 *                    the reference calls scipy.spatial.ConvexHull(points).volume; 0.0 for a degenerate hull)
 *   variance_inv[E]  1000 if var(z) < 1e-6 else 0.001/var(z)                     (cloth_env.py:1075-1084)
 *   oob[E]           out-of-bounds test with slack 0.25 on x,y and [0,1) on z    (cloth_env.py:1020-1045)
 *   tear[E]          Cloth.have_tear
 * Any pointer may be NULL. */
int clothhip_metrics(clothhip_handle *h, double *coverage, double *variance_inv, uint8_t *oob, uint8_t *tear);
/* the same plus n_below_half_thickness[E] = #points with z < thickness/2, the numerator of the 'height' reward's
 * compute_height (cloth_env.py:603-609) */
int clothhip_metrics_ex(clothhip_handle *h, double *coverage, double *variance_inv, uint8_t *oob, uint8_t *tear,
                        int32_t *n_below_half_thickness);
/* the same hull-area routine on caller-supplied points xy[n][2] (pure host function; used by tests to pin it
 * against scipy's Qhull on the golden states) */
double clothhip_hull_area(const double *xy, int32_t n);

/* Device-resident observation path for the multi-GPU driver: writes the '1d' observation
 * (cloth_env.py:196-200: [x0,y0,z0,x1,...] per env) of every env as float32 into a DEVICE buffer
 * d_out[E][3P] (e.g. a torch/RCCL gather buffer). Asynchronous on the handle's stream. */
int clothhip_write_obs_f32_device(clothhip_handle *h, void *d_out);
/* Same, schedules read from a DEVICE array of ClothSchedule[E] (e.g. after an RCCL broadcast). */
int clothhip_run_device_sched_async(clothhip_handle *h, const void *d_sched);
/* Headless RGB / depth rendering of every env's cloth mesh: what the reference obtains by exporting the
 * particle grid as a triangle mesh (cloth_env.py:218-229) and calling a Blender subprocess
 * (gym_cloth/blender/get_image_rep_279.py; cloth_env.py:212-330). The scene follows that script -- pinhole camera
 * (default: at (0.5, 0.5, 1.45) looking straight down, lens 40 mm on a 36 mm sensor), the two cloth sides in different
 * colours, a shadow-less lamp, a white bed plane -- but the pixels are this library's own rasterisation rules
 * (csrc/cloth_render.hpp), pinned to a numpy restatement (oracle/render_oracle.py), not to Blender. */
typedef struct ClothRenderParams {
    int32_t width, height;           /* cfg: 224 x 224 (cloth_env.py:152-157) */
    float cam_pos[3];                /* 0.5, 0.5, 1.45 (+ dom_rand camera_pos) */
    float world_to_cam[9];           /* row-major rotation; the camera looks along -z_cam with +y_cam up. Identity = straight
                                        down, image +x = world +x, image up = world +y. (Blender's rotation_euler XYZ of
                                        get_image_rep_279.py:119-122 is camera-to-world = Rz Ry Rx: pass its transpose.) */
    float lens_mm, sensor_mm;        /* 40, 36 */
    float front[3], back[3];         /* (0.070, 0.050, 0.600), (0.070, 0.300, 0.900) */
    float background[3];             /* bed plane, (1, 1, 1) */
    float light_dir[3];              /* unit vector towards the lamp */
    float ambient, energy;
} ClothRenderParams;
/* rgb: [E][height][width][3] uint8 or NULL; depth: [E][height][width] float32 camera-space depth (distance along the view
 * axis; the bed plane where no cloth is) or NULL; swap_sides[E] or NULL: != 0 swaps the two side colours (a tier-2 cloth
 * with init_side False, get_image_rep_279.py:235-239). */
int clothhip_render(clothhip_handle *h, const ClothRenderParams *params, const uint8_t *swap_sides, uint8_t *rgb,
                    float *depth);

/* (additive, ABI 7) Finished uint8 image observations of n cloths in one call: the observation type the reference's shipped
 * configurations train on (t{1,2,3}_rgbd.yaml; ClothEnv.state with obs_type 'blender', cloth_env.py:196-209), for every slot of
 * an episode launch at once. Same scene and pixel rules as clothhip_render -- every image equals, byte for byte, what
 * clothhip_render gives for the same float32 positions, finished as below -- but the z-buffer lives in LDS, band of rows by band
 * (csrc/cloth_render_obs.hpp), the image is finished on the device, and the device scratch is that of a fixed chunk of images
 * whatever n is.
 *   format: CLOTHHIP_IMG_RGB [H][W][3]; CLOTHHIP_IMG_DEPTH [H][W][3], the 8-bit depth replicated (cloth_env.py:207-209);
 *           CLOTHHIP_IMG_RGBD [H][W][4] (:202-205). The 8-bit depth of a pixel of camera-space depth d, in float32:
 *           lo, hi = min, max of d over the image; nz = hi > lo ? (d - lo) / (hi - lo) : 0; d8 = max(0, rint(nz * 255) - 50)
 *           (get_image_rep_279.py:390-406, cloth_env.py:301-302; rint rounds half to even).
 *   source: where the n cloths come from, each converted to float32 as clothhip_render converts the state.
 *   valid[n] or NULL (= all): an image with valid[i] == 0 is not rasterised, its bytes are zero.
 *   swap[n] or NULL: != 0 swaps the two side colours of image i (a tier-2 cloth with init_side False).
 *   out: host [n][H][W][C] or NULL; d_out: device buffer of the same layout on the handle's device, or NULL. With d_out the images
 *   are rendered into it (and copied to out as well when both are given); byte offsets are 64-bit.
 * Runs on the handle's stream and returns when out is filled / the work on d_out has completed.
 * CLOTHHIP_EINVAL: n does not match the source, unknown format or source, the image-size or lens rules of clothhip_render, an
 * image too wide for a one-row band in LDS beside the grid, CLOTHHIP_OBS_HOST without obs_host. CLOTHHIP_ESTATE:
 * CLOTHHIP_OBS_SLOTS / CLOTHHIP_OBS_RESETS before any clothhip_run_actions launch, between its _begin and _end, or when the last
 * launch was not given want_obs / want_reset_obs (the tables stay resident until the next launch). A failed call writes
 * nothing; n == 0 succeeds. */
enum { CLOTHHIP_IMG_RGB = 0, CLOTHHIP_IMG_DEPTH = 1, CLOTHHIP_IMG_RGBD = 2 };
enum { CLOTHHIP_OBS_STATE = 0,   /* the handle's particles, n == E */
       CLOTHHIP_OBS_SLOTS = 1,   /* obs table of the last run_actions launch, n == T*E, image i = slot [t][e] */
       CLOTHHIP_OBS_RESETS = 2,  /* its reset_obs table, n == E*n_scripts, image i = [e][k] */
       CLOTHHIP_OBS_HOST = 3 };  /* obs_host[n][3P] float32, uploaded */
int clothhip_render_obs(clothhip_handle *h, const ClothRenderParams *p, int32_t source, const float *obs_host,
                        int64_t n, const uint8_t *valid /*[n] or NULL = all*/, const uint8_t *swap /*[n] or NULL*/,
                        int32_t format, uint8_t *out /*host [n][H][W][C] or NULL*/, void *d_out /*device, same layout, or NULL*/);

/* Raw device buffers on the handle's device, for the multi-GPU driver's RCCL staging (action tables in, result /
 * observation tables out; gym_cloth_amd/dist.py). upload/download run on the handle's stream and synchronise it, so
 * they are ordered with the stepper launches. */
int clothhip_device_alloc(clothhip_handle *h, uint64_t nbytes, void **d_out);
int clothhip_device_free(clothhip_handle *h, void *d);
int clothhip_device_upload(clothhip_handle *h, void *d_dst, const void *src, uint64_t nbytes);
int clothhip_device_download(clothhip_handle *h, void *dst, const void *d_src, uint64_t nbytes);
/* the handle's hipStream_t as an opaque pointer (for event timing / stream ordering by the caller) */
void *clothhip_stream(clothhip_handle *h);

/* Timing of the last clothhip_run/_async/_update launch measured with HIP events recorded on the
 * handle's stream around the stepper kernel: milliseconds, or a negative value if none. */
double clothhip_last_kernel_ms(clothhip_handle *h);

/* (new, ABI 5) Which compiled stepper variant the handle's LAST launch ran (clothhip_run*, clothhip_update, clothhip_run_actions*),
 * so that tests and the benchmark can tell the variants apart instead of inferring them from the batch size:
 *   v[0] threads per cloth, v[1] particles per thread, v[2] table mode: 1 strain-sweep window table resident in LDS, 0 streamed
 *   from L2 (standard arithmetic; with v[4] the fp32 LEAN build compiled for three cloths per CU, or the fp64 LEAN build), and LEAN only:
 *   -1 / -2 / -3 compiled for four / five / six cloths per CU, 2 the table in LDS plus per-point slots (eight waves per cloth),
 *   3 a large grid with the whole CU for one cloth, 4 two large-grid cloths per CU (names: csrc/stepper_traits.hpp),
 *   v[3] rest lengths in registers / LEAN flag as compiled (0/1), v[4] 1 when the LEAN arithmetic ran (gather stencil recomputed,
 *   rest lengths from the three-value palette), v[5] episode-loop flavour (0 plain schedule, 1 flat-tier episodes, 2 + tier-2 /
 *   highest-point code), v[6] dynamic LDS bytes per cloth, v[7] cloths resident per CU for that kernel and LDS size
 *   (hipOccupancyMaxActiveBlocksPerMultiprocessor), v[8] compute units of the device, v[9] precision (0 f64, 1 f32).
 * Returns CLOTHHIP_ESTATE when the handle has not launched a stepper yet. */
int clothhip_last_variant(clothhip_handle *h, int32_t v[10]);

/* (new, ABI 7) Kernel dispatches the handle's last stepper launch was issued as: 1, or -- a time-sliced clothhip_run_actions over more
 * cloths than are resident -- one per generation of resident cloths (rocprofv3 lists them one by one; clothhip_last_kernel_ms spans
 * them all). CLOTHHIP_ESTATE before the first launch. */
int clothhip_last_dispatches(clothhip_handle *h, int32_t *n);

/* (new, ABI 7) 25 or 50 when the handle's last stepper launch ran a GRID-SPECIALISED build of the variant clothhip_last_variant names -- the
 * kernel compiled with the 25x25 grid of the shipped configurations (cfg/t1_rgbd.yaml:15-16) or the 50x50 grid of BASELINE configs[4] as
 * compile-time constants: particle count, LDS carve-up, hash- and window-table sizes --, 0 for the generic build (any grid). Same arithmetic,
 * same results bit for bit (tests/test_gpu_lean.py, tests/test_gpu_fullsize.py); CLOTHHIP_DEBUG_NOSPEC=1 at launch time forces the generic build. */
int clothhip_last_specialised(clothhip_handle *h, int32_t *n_side);

/* (new, ABI 7; measurement only, NOT a reference path) on != 0: THIS handle's clothhip_run_actions launches run the relaxed-order
 * companion kernel -- self-collision in Jacobi order, strain limit in coloured order (cloth.pyx:258-296 and :313-343 keep list order;
 * this does not) -- so that bench.py can state what the reference's Gauss-Seidel orders cost. Its trajectories are not the
 * reference's; clothhip_last_variant reports flavour v[5] == 3 for such a launch. Per handle (round 5 read an environment variable at
 * create time, which leaked into every handle created meanwhile). Only the eight-wave LEAN layout has the companion (fp32, flat tiers,
 * 25x25 class, <= 512 cloths): other handles get CLOTHHIP_ESTATE from clothhip_run_actions*. update() / step() on the handle stay exact. */
int clothhip_set_relaxed_order(clothhip_handle *h, int32_t on);

/* Diagnostics of the last clothhip_run*: stats[E][16]: [0..3] = {strain sweeps run, 64-spring windows walked, passes
 * over a window, passes in which a correction was applied}; [15] = shader clocks/1024 the env's whole schedule
 * took; in the profiling build of the library (make -C gym_cloth_amd/csrc stamps) with CLOTHHIP_DEBUG_PHASES bit 32
 * set, [4..15] = shader cycles/64 per kernel phase instead. Not part of the reference surface. */
int clothhip_debug_stats(clothhip_handle *h, int32_t *stats);

/* Arithmetic self-test used by the parity tests: evaluates out[i] = op(a[i], b[i]) in double ON THE
 * DEVICE with the same compiler flags as the stepper (op 0: a/b, 1: sqrt(a), 2: a*b+c unfused = (a*b)+b,
 * 3: floor(a/b)).  Lets tests assert IEEE-correct rounding of the device's sqrt/div bit-for-bit. */
/* (new, host only) The static tables of the strain sweep for a grid, for the CPU test that pins the sweep's pass rule to the
 * sequential loop of cloth.pyx:258-296: `spring_at[slot]` = reference list index of the spring in window-table slot `slot`
 * (-1: empty), `ent[slot]` = packed entry (ptA | ptB << 12 | level-in-window << 24 | reach << 28), `dep[slot]` = the lanes of
 * the slot's 64-slot window whose springs it transitively depends on. Arrays hold `capacity` slots; returns CLOTHHIP_EINVAL
 * when that is too small (n_slots is set either way). Any array may be NULL. */
int clothhip_selftest_windows(const ClothParams *params, int32_t *n_windows, int32_t *n_slots, int32_t *reach_shift,
                              int32_t *spring_at, uint32_t *ent, uint64_t *dep, int32_t capacity);

/* Host-side view of the variant / LDS-layout decisions clothhip_create takes for (params, precision, n_envs) on a device of n_cus
 * compute units -- no device needed (ABI 6). out[24]: [0..9] the standard layout {threads per cloth, particles per thread, table mode,
 * rest lengths in registers, cell-ordered copy, LDS bytes, hash-table slots, LDS the in-kernel metrics of clothhip_run_actions can
 * borrow, LDS they need, 1 if that fits}; [10] 1 if a LEAN layout exists beside it, [11] the cloths per CU it is built for;
 * [12..21] the LEAN layout, same fields; [22] what clothhip_fused_supported would return; [23] 1 if the layout fits the CU's LDS. */
int clothhip_selftest_layout(const ClothParams *params, int32_t precision, int32_t n_envs, int32_t n_cus, int32_t *out, int32_t capacity);

/* Host-side self-test of csrc/cloth_rng.hpp (the same functions the kernel runs): n draws of kind 0 next32, 1 rand(),
 * 2 uniform(a, b), 3 randint((uint32)a), 4 _randval_minabs(a, b, minabs = c) into out[n]; kind 5 skips (uint64)a words.
 * state[625] = key[624], pos: numpy RandomState.get_state()[1:3], advanced in place. No device needed. */
int clothhip_selftest_rng(uint32_t *state, int32_t kind, int32_t n, double a, double b, double c, double *out);

/* Host-side self-tests of clothhip_render_obs; no device needed.
 * _depth8: the finishing rule of its DEPTH / RGBD formats, through the same inline function the kernel runs (csrc/cloth_render_obs.hpp
 * depth8): depth[n_images][npx] float32 camera-space depth -> out[n_images][npx], lo / hi taken per image.
 * _render_plan: the band plan for a params->n_side grid and a width x height image: out[4] = {rows per band, bands per image,
 * dynamic LDS bytes per workgroup, 1 if it fits}; 0 in the last entry: not even a one-row band fits beside the grid's per-vertex arrays
 * (out[2] is then what that band would need) and clothhip_render_obs returns CLOTHHIP_EINVAL for that size. */
int clothhip_selftest_depth8(const float *depth, int32_t n_images, int64_t npx, uint8_t *out);
int clothhip_selftest_render_plan(const ClothParams *params, int32_t width, int32_t height, int32_t out[4]);
/* Host-side self-test of PPO's exponential (PPO ON THE DEVICE above): out[i] = exp_fixed(x[i]), the inline function the two surrogate kernels run,
 * k_fit_loss_ppo (the ONE fixed-sigma kernel, of the shared network and of population rows) and k_fit_loss_ppo_sigma
 * (csrc/cloth_exp_fixed.hpp), computed on the host; no device needed. CLOTHHIP_EINVAL for n < 0, a NULL table with n > 0 or a NaN. */
int clothhip_selftest_exp_fixed(const double *x, int64_t n, double *out);
/* Host-side self-test of the exploration noise's variate (EXPLORATION NOISE ON THE DEVICE above): out[i][0..3] = normal_fixed(seed, env[i],
 * slot[i]), the inline function k_policy_noise_fill runs (csrc/cloth_philox.hpp), computed on the host; no device needed.
 * CLOTHHIP_EINVAL for n < 0 or a NULL table with n > 0. */
int clothhip_selftest_normal_fixed(uint64_t seed, const uint32_t *env, const uint64_t *slot, int64_t n, double *out);
int clothhip_selftest_arith(int32_t device, int32_t op, const double *a, const double *b, double *out,
                            int64_t n);

#ifdef __cplusplus
}
#endif
#endif
