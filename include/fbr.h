/*
 * fbr.h -- C-ABI of libfbr (FloBaRoID regressor hot path on MI355X / gfx950).
 *
 * The reference has no FFI of its own for this path: its per-sample arithmetic is reached through
 * iDynTree's SWIG bindings and its reductions through NumPy/SciPy.  Every entry point below names
 * the reference call site(s) it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; int return: 0 = OK, negative = error (fbr_last_error()).
 *   - All numeric data is IEEE fp64, C-contiguous, row-major.
 *   - Every data pointer carries a memory-space flag: FBR_HOST (pageable/pinned host memory; the call
 *     stages it through the device) or FBR_DEVICE (HIP device memory on the model's device).
 *   - Calls are blocking: results are complete (and the model's stream synchronised) on return.
 *   - A model handle may be used from one host thread at a time; handles are per-process and must be
 *     created after fork() (the reference's multiprocessing users build one Model per worker,
 *     excitation/analyticalGradient.py:188-210).
 *   - There is NO CPU fallback: without a usable HIP device every compute call fails with FBR_E_NODEVICE.
 */
#ifndef FBR_H
#define FBR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBR_OK 0
#define FBR_E_INVALID (-1)   /* bad argument */
#define FBR_E_NODEVICE (-2)  /* no HIP device / HIP runtime failure at init */
#define FBR_E_HIP (-3)       /* HIP runtime error during the call */
#define FBR_E_UNSUPPORTED (-4)
#define FBR_E_FORK (-5)      /* handle / HIP runtime inherited through fork(): create the model in the process that uses it */

#define FBR_HOST 0
#define FBR_DEVICE 1

typedef struct fbr_model fbr_model; /* opaque */

/*
 * Kinematic tree + identified-column layout.  Replaces what the reference pulls out of
 * iDynTree::ModelLoader / Model (identification/model.py:60-68,112-131) and the layout logic of
 * Model.__init__ (model.py:134-168).  Links and DOFs are indexed as the caller serialises them (any order: parents
 * need not precede children); flobaroid_amd/topology.py hands over iDynTree's traversal order, the one the reference's
 * linkNames / jointNames follow (model.py:86-94,121-127).  Columns of the regressor are link-major, 10 per link
 * [m, m*cx, m*cy, m*cz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz] (model.py:220-231), followed by the friction
 * blocks Fc | Fv (or Fv+,Fv-) | off | Fs (model.py:459-503).
 */
typedef struct {
    int32_t num_links;
    int32_t num_dofs;
    const int32_t *parent;    /* [L] parent link, -1 for the base */
    const int32_t *dof_index; /* [L] DOF of the joint to the parent, -1 when fixed / base */
    const double *rest_R;     /* [L][9] child orientation in the parent frame at q = 0 */
    const double *rest_p;     /* [L][3] child origin in the parent frame */
    const double *axis;       /* [L][3] unit joint axis in the child frame (rotation axis / sliding direction) */
    int32_t floating_base;    /* opt['floatingBase']: rows per sample = num_dofs + 6 */
    double gravity[3];        /* reference: (0, 0, -9.81), model.py:182-187 */
    int32_t friction;           /* opt['identifyFrictionSimultaneously'] */
    int32_t friction_symmetric; /* opt['identifySymmetricVelFriction'] */
    int32_t gravity_only;       /* opt['identifyGravityParamsOnly'] (keeps 4 columns per link) */
    double stribeck_velocity;   /* opt['stribeckVelocity'] (> 0 adds the Fs block) */
    const int32_t *joint_type;  /* [L] type of the joint to the parent for links with a DOF: 1 revolute / continuous, 2 prismatic (other
                                   entries ignored); NULL: every DOF is revolute.  iDynTree's loader takes any URDF (model.py:60-67) */
} fbr_topology;

/*
 * A batch of trajectory samples = what Model.computeRegressors reads per sample_index
 * (model.py:374-394, 425-439, 462).  All arrays share the same memory space.
 */
typedef struct {
    int64_t num_samples;
    int32_t mem;            /* FBR_HOST or FBR_DEVICE */
    const double *q;        /* [S][n] positions */
    const double *dq;       /* [S][n] velocities */
    const double *ddq;      /* [S][n] accelerations */
    const double *base_vel; /* [S][6] base twist [lin; ang], mixed representation (floating base) */
    const double *base_acc; /* [S][6] its time derivative */
    const double *base_rpy; /* [S][3] rpy with world_T_base = Transform(RPY(rpy),0).inverse() */
    const double *sign;     /* [S][n] Coulomb sign term (helpers.getFrictionSignSeries); NULL unless friction */
} fbr_states;

/* ---- library / device ------------------------------------------------------------------------- */
/* Version of THIS header.  fbr_version() returns the value the loaded library was built with: a caller compares the two before its first
 * call (flobaroid_amd/_lib.py load_library refuses a mismatch), because the C-ABI has grown in place -- 101: fbr_topology.joint_type,
 * the num_samples argument of fbr_gram_program_info / fbr_model_link_merge_info, option "fused_id"; 102: fbr_gram_lane_info, options
 * "gram_lane" / "gram_force_tiles"; 103: fbr_candidate_extrema; 104: fbr_model_set_capsules, fbr_candidate_capsule_distances, and -- added under the same number, which
 * tests/test_capsule_abi.py pins: two new entry points, no existing signature, struct or array size changed -- fbr_regressor_weights,
 * fbr_fourier_gradient; and, in the same way, fbr_capsule_distance_gradients, fbr_fourier_position_chain; fbr_torque_row_sweep,
 * fbr_fourier_state_chain; fbr_suspended_base_motion, fbr_suspended_records; fbr_model_set_boxes, fbr_candidate_box_distances;
 * fbr_box_distance_gradients; fbr_model_set_hulls, fbr_candidate_hull_distances; fbr_hull_distance_gradients; fbr_model_set_hull_meshes;
 * fbr_mesh_distance_gradients; fbr_model_set_large_hulls, option "hull_large_all"; fbr_large_hull_distance_gradients, option
 * "hull_grad_tile"; fbr_model_set_large_hull_meshes; fbr_large_mesh_distance_gradients, option "mesh_grad_order"; fbr_dopt_terms (with FBR_MAX_DOPT_COLUMNS);
 * fbr_dopt_observability. */
#define FBR_VERSION 104
int fbr_version(void);
int fbr_device_count(void);        /* number of visible HIP devices (0 if none / no runtime) */
const char *fbr_last_error(void);  /* thread-local message of the last failing call */

/* ---- model ------------------------------------------------------------------------------------ */
/* Builds device tables for `topo` on HIP device `device`.  Replaces ModelLoader.loadModelFromFile +
   KinDynComputations.loadRobotModel (model.py:60-68). */
int fbr_model_create(const fbr_topology *topo, int device, fbr_model **out);
void fbr_model_destroy(fbr_model *m);
/* rows per sample (N_OUT, model.py:102-105) and identified columns (num_identified_params, model.py:138-168) */
int fbr_model_dims(const fbr_model *m, int32_t *rows_per_sample, int32_t *num_cols);
/* Run subsequent calls on this hipStream_t (e.g. torch's current stream); NULL = the model's own stream. */
int fbr_model_set_stream(fbr_model *m, void *hip_stream);

/* ---- per-sample kernels ----------------------------------------------------------------------- */
/*
 * Stacked standard regressor, Y_out [S*rows][cols] -- the reference's regressor_stack
 * (model.py:349-354, 435-523: setRobotState + inverseDynamicsInertialParametersRegressor + friction
 * column blocks + gravity-only column deletion, one Python iteration per sample).
 */
int fbr_regressor_batch(fbr_model *m, const fbr_states *st, double *Y_out, int32_t out_mem);

/*
 * Generalized torques [base wrench(6); joint torques] per sample, tau_out [S][rows], from the full
 * standard parameter vector x_std (host pointer; 10 per link + friction slots laid out as in
 * model.py:134-168) -- Model.simulateDynamicsIDynTree (model.py:239-331): KinDynComputations.
 * inverseDynamics plus the friction model sign*Fc + Fv*dq + off (+ Stribeck with vel_sign, may be NULL).
 */
int fbr_inverse_dynamics_batch(fbr_model *m, const fbr_states *st, const double *x_std, int32_t num_x,
                               const double *vel_sign, double *tau_out, int32_t out_mem);

/*
 * Per-candidate extrema of the trajectory optimiser's constraints (excitation/trajectoryOptimizer.py objectiveFunc: g and the soft costs,
 * and the sample indices its analytical gradient caches) without the torques leaving the device.  The states are ncand equal candidates
 * of T = num_samples / ncand consecutive samples (the layout of fbr_gram_grouped / fbr_fourier_states); x_std, vel_sign and the sign
 * series as for fbr_inverse_dynamics_batch, whose torques -- bit for bit, on the same route -- are the ones reduced.
 *   val_out [ncand][4][n], idx_out [ncand][4][n] (out_mem): quantity 0 min q, 1 max q, 2 max |dq|, 3 max |nan_to_num(tau)| over the
 *   joint rows (fb .. fb+n-1: the base wrench is skipped); the index is the sample inside its candidate (0 .. T-1).  NumPy's rules:
 *   ties go to the first sample, a NaN in q / dq is the value and its first occurrence the index; in tau NaN counts as 0, +-inf as DBL_MAX.
 * FBR_E_INVALID: ncand < 1, num_samples 0 or not a multiple of ncand, x_std too short, Stribeck without vel_sign.
 */
int fbr_candidate_extrema(fbr_model *m, const fbr_states *st, int32_t ncand, const double *x_std, int32_t num_x,
                          const double *vel_sign, double *val_out, int64_t *idx_out, int32_t out_mem);

/*
 * Joint torque rows of chosen samples under the finite-difference sweep of the analytical gradient's torque Jacobians (excitation/
 * analyticalGradient.py:114-183: 1 + 3 n inverse dynamics at the sample where |tau_n| peaks; Phase C, lines 764-953, chains their forward
 * differences).  The states are ncand equal candidates of T = num_samples / ncand samples (the layout of fbr_candidate_extrema); x_std,
 * vel_sign and the sign series as for fbr_inverse_dynamics_batch.  sample [ncand][nrows] (int64, 0 .. T-1: the sample inside the candidate)
 * and joint [ncand][nrows] (int32, 0 .. n-1; NULL: nrows == n and joint = column index) live in st->mem.
 *   out [ncand][nrows][1 + 3 n] (out_mem): joint torque row fb + joint of the inverse dynamics of x_std -- entry 0 at the state of the
 *   sample, entry 1 + kind * n + d with +eps on q_d (kind 0) / dq_d (1) / ddq_d (2): the entry order of fbr_fd_scores.  Held at the
 *   sample's own values, as in the reference: the sign series, vel_sign (the Stribeck exponent) and the base state; the viscous term moves
 *   with dq.  One lane per evaluation on the route of fbr_inverse_dynamics_batch (merged links included), nothing expanded in memory; the
 *   two-kernel form expands chunk by chunk (option "fused_id" 0, joint paths beyond 24 joints, more than 105 DOF).  No atomics: the same
 *   bits on every run.
 * FBR_E_INVALID: as for fbr_candidate_extrema, nrows < 1, joint == NULL with nrows != n, eps zero or not finite, and a sample or joint
 * index out of range (read clamped on the device, never out of bounds, and reported after the call; out is then unspecified).
 */
int fbr_torque_row_sweep(fbr_model *m, const fbr_states *st, int32_t ncand, int64_t nrows, const int64_t *sample, const int32_t *joint,
                         const double *x_std, int32_t num_x, const double *vel_sign, double eps, double *out, int32_t out_mem);

/*
 * Base motion of candidate trajectories of a robot that hangs from a ball joint at the origin O of link att_link -- the reference's
 * simulate_suspended_base_motion (excitation/suspendedDynamics.py; called by simulateTrajectory, excitation/trajectoryGenerator.py:171-187,
 * on every objective evaluation under floatingBaseAttachment "suspended": one Python iteration per sample, each with a mass matrix and an
 * inverse dynamics from iDynTree).  The states are ncand equal candidates of T = num_samples / ncand consecutive samples (the layout of
 * fbr_candidate_extrema), in host or device memory; only q, dq, ddq are read.  x_std: the full standard parameter vector (host) as for
 * fbr_inverse_dynamics_batch; its inertial part (10 per link) is used, no friction.  att_link: a link in the caller's numbering (the
 * UNMERGED links, like the capsules' links) -- the base itself, a moving link or one behind fixed joints.  Gravity is the model's.
 * Per candidate, line for line:
 *   equilibrium search at sample 0 with zero velocities: at most FBR_SUSP_EQ_MAX_ITER iterations rpy -= FBR_SUSP_EQ_STEP * moment, clipped to
 *     +-FBR_SUSP_EQ_CLIP_DEG, until |moment| < FBR_SUSP_EQ_TOL;
 *   for t = 0 .. T-1: solve (M_bb_rot + damping dt 1) alpha = -(M_bj ddq + h_b)_rot - damping omega; record the base link's pose and twist;
 *     then (t < T-1) omega += alpha dt, rpy += rpy_rates(rpy, omega) dt (angular_velocity_to_rpy_rates as written), each angle clamped to
 *     +-FBR_SUSP_MAX_SWING_DEG, its velocity multiplied by FBR_SUSP_BOUNCE when it points outwards.
 * Outputs (out_mem), S = num_samples:
 *   base_rpy [S][3]  rpy of the INVERSE of world_R_base (the convention of fbr_states.base_rpy; Rotation.RPY = Rz(y) Ry(p) Rx(r)), by
 *                    r = atan2(R21, R22), p = asin(-R20), y = atan2(R10, R00); at |R20| >= 1: p = +-pi/2, r = 0, y = atan2(-R01, R11)
 *   base_pos [S][3]  base link origin in the world frame, the attachment at the origin
 *   base_vel [S][6]  mixed twist [lin; ang]
 *   base_acc [S][6]  central differences of base_vel with dt, one-sided at a candidate's two ends; all zeros when T <= 2
 *   att_state [S][6] or NULL: the attachment's rpy and angular velocity (world) as used at each step
 *   info [ncand][2] or NULL: moment evaluations of the equilibrium search (FBR_SUSP_EQ_MAX_ITER: not converged), clamp events
 * Two kernels (csrc/fbr_kinid.h): one lane per sample reduces the sample to a record of 39 doubles (the composite inertia, Coriolis
 * coupling, joint-motion moment and first mass moment about O, the base link's pose and twist relative to the attachment); one lane per
 * candidate then steps through its records at O(1) per step.  A candidate's result does not depend on the rest of the batch; no atomics:
 * the same bits on every run.  NaN inputs give NaN outputs.
 * FBR_E_INVALID: a model without a floating base, att_link out of range, dt not finite or <= 0, damping not finite or < 0, ncand < 1,
 * num_samples 0 or not a multiple of ncand, x_std shorter than 10 per link.  FBR_E_UNSUPPORTED: the lane kernels do not serve the model
 * (option "fused_id" 0, or joint paths of more than 24 joints); there is no two-kernel form.
 */
#define FBR_SUSP_EQ_MAX_ITER 200
#define FBR_SUSP_EQ_TOL 0.01
#define FBR_SUSP_EQ_STEP (1.0 / 700.0)
#define FBR_SUSP_EQ_CLIP_DEG 30.0
#define FBR_SUSP_MAX_SWING_DEG 25.0
#define FBR_SUSP_BOUNCE (-0.3)
int fbr_suspended_base_motion(fbr_model *m, const fbr_states *st, int32_t ncand, const double *x_std, int32_t num_x, int32_t att_link, double dt,
                              double damping, double *base_rpy, double *base_pos, double *base_vel, double *base_acc, double *att_state,
                              int64_t *info, int32_t out_mem);

/*
 * Capsule collision geometry of the robot, for fbr_candidate_capsule_distances: the reference's collisionMode "capsule"
 * (excitation/capsule.py: a capsule is a segment in a link's frame plus a radius; optimizer.py self._capsules, trajectoryOptimizer.py
 * self._collision_pairs).  Host arrays, copied:
 *   link [ncaps]      index of the capsule's link in the topology as the caller serialised it -- the UNMERGED links: a link attached by a
 *                     fixed joint keeps its own capsule (the column reductions of "link_merge" play no part in this path)
 *   seg [ncaps][6]    p0 | p1 in that link's frame (p0 == p1: a sphere)
 *   radius [ncaps]
 *   pairs [npairs][2] indices into the CAPSULE list (not link indices); the pairs kernel keeps a pair's first capsule in registers while it
 *                     does not change, so a list sorted by its first entry (the reference's order) is the cheapest
 * A second call replaces the set; ncaps = 0 clears it.  At most FBR_MAX_CAPSULES capsules and FBR_MAX_CAPSULE_PAIRS pairs (WALK-MAN: 48
 * links, 1 128 link pairs).  FBR_E_INVALID: more than that, a link or a pair index out of range, a capsule paired with itself, a negative
 * or non-finite radius, a non-finite endpoint; the set in place before a refused call stays.
 */
#define FBR_MAX_CAPSULES 4096
#define FBR_MAX_CAPSULE_PAIRS 262144
int fbr_model_set_capsules(fbr_model *m, int32_t ncaps, const int32_t *link, const double *seg, const double *radius, int32_t npairs,
                           const int32_t *pairs);

/*
 * Per candidate and capsule pair, the smallest capsule distance over the candidate's checked samples -- the collision block of
 * objectiveFunc in capsule mode (excitation/trajectoryOptimizer.py "check collision constraints": setCollisionRobotState per checked
 * sample, capsule_distance per pair, `if d < g[...]`) for the main-trajectory samples, without a pose leaving the device.
 * The states are ncand equal candidates of T = num_samples / ncand consecutive samples (the layout of fbr_candidate_extrema); only q and,
 * on a floating-base model, base_rpy are read (dq, ddq and the twists may be NULL).  base_pos [S][3] (st->mem space) or NULL (zero): the
 * base sits at world_T_base = Transform(RPY(base_rpy).inverse(), base_pos), the reference's setCollisionRobotState; fixed base, or
 * base_rpy NULL: identity.  The samples t = 0, step, 2 step, ... < T of every candidate are checked (collisionCheckStep).
 *   dist_out [ncand][npairs]  min over t of |closest_a - closest_b| - r_a - r_b (negative: the capsules overlap)
 *   idx_out [ncand][npairs]   the sample index inside the candidate where it is reached
 * The reference's rules: the comparison is a strict < walking t upwards from 1e10, so the first sample wins a tie, a NaN distance never
 * wins, and a pair for which no sample wins returns 1e10 and index -1.  Margins (a constant per pair) are the caller's.  No atomics: the
 * same bits on every run.
 * FBR_E_INVALID: no capsule set or one without pairs, ncand < 1, step < 1, num_samples 0 or not a multiple of ncand.
 */
int fbr_candidate_capsule_distances(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, int32_t step,
                                    double *dist_out, int64_t *idx_out, int32_t out_mem);

/*
 * Box collision geometry, for fbr_candidate_box_distances: the pairs of the reference's collision block that go to fcl.distance on the box
 * fallback of optimizer.py _getLinkCollisionGeometry -- every pair of collisionMode "box", and in collisionMode "capsule" every pair with a
 * world link or with a robot link that has no capsule.  Independent of the capsule set: both can be in place at once.  Host arrays, copied:
 *   link [nboxes]       index of the box's link among the UNMERGED links (as for fbr_model_set_capsules), or -1: a world box, fixed in space
 *   half [nboxes][3]    half extents along the box axes (positive, finite)
 *   center [nboxes][3]  robot box: the centre's offset from the link origin, see center_in_link_axes; world box: the centre in the world
 *   rot [nboxes][9]     row-major, columns = box axes; read for world boxes only (a robot box has its link's axes); may be NULL without any
 *   center_in_link_axes 0: a robot box sits at p_link + center, the offset added in WORLD axes (the reference's Transform(rot, pos + offset));
 *                       1: at p_link + R_link center, the geometrically correct placement
 *   pairs [npairs][2]   indices into the BOX list; a pair's first box stays in registers while it does not change
 * A second call replaces the set; nboxes = 0 clears it.  FBR_E_INVALID: more than FBR_MAX_BOXES boxes or FBR_MAX_BOX_PAIRS pairs, a link or a
 * pair index out of range, a box paired with itself, a pair of two world boxes, a world box without rot, a non-positive or non-finite half
 * extent, a non-finite centre or rotation; the set in place before a refused call stays.
 */
#define FBR_MAX_BOXES 4096
#define FBR_MAX_BOX_PAIRS 262144
int fbr_model_set_boxes(fbr_model *m, int32_t nboxes, const int32_t *link, const double *half, const double *center, const double *rot,
                        int32_t center_in_link_axes, int32_t npairs, const int32_t *pairs);

/*
 * Per candidate and box pair, the smallest signed box distance over the candidate's checked samples and the sample index where it is
 * reached: states, base_pos, ncand, step, outputs and the comparison rules (strict < from 1e10, first sample wins a tie, a NaN never wins,
 * 1e10 / -1 when no sample wins, the same bits on every run) exactly as for fbr_candidate_capsule_distances.
 *   dist_out [ncand][npairs]  separated boxes: their exact Euclidean distance; touching or overlapping: the largest (least negative) gap over
 *                             the 15 separating axes, i.e. minus the minimum translation that separates them (cross axes of squared length
 *                             below 1e-12 are skipped).  The reference's FCL returns a GJK distance of tolerance 1e-6 and a build-dependent
 *                             negative value: the sign agrees.
 * FBR_E_INVALID: no box set or one without pairs, ncand < 1, step < 1, num_samples 0 or not a multiple of ncand.
 */
int fbr_candidate_box_distances(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, int32_t step, double *dist_out,
                                int64_t *idx_out, int32_t out_mem);

/*
 * Convex-hull collision geometry, for fbr_candidate_hull_distances: the reference's default collisionMode "convex", in which every pair of
 * the collision block goes to fcl.distance on the convex hull of the link's mesh (links without a mesh and all world links: a box, here a
 * hull of 8 vertices).  Independent of the capsule and the box set.  Host arrays, copied; the tables of hull h are rows
 * [vbeg[h], vbeg[h + 1]) of verts, [fbeg[h], fbeg[h + 1]) of planes and [ebeg[h], ebeg[h + 1]) of edges:
 *   link [nhulls]       index of the hull's link among the UNMERGED links, or -1: a world hull, fixed in space
 *   offset [nhulls][3]  origin of the hull's axes: an offset from the link origin (see offset_in_link_axes), or the world position (link -1)
 *   rot [nhulls][9]     row-major rotation of a world hull; ignored for a robot hull, which has the axes of its link; may be NULL
 *                       when there is no world hull
 *   offset_in_link_axes 0: a robot hull sits at p_link + offset, the offset added in WORLD axes (the reference's Transform(rot, pos + offset));
 *                       1: at p_link + R_link offset
 *   verts [][3]         the vertices in the hull's axes (4 to FBR_MAX_HULL_VERTICES a hull: the edge-pair pass of an overlapping pair is
 *                       E_A E_B arc tests, E <= 3 V - 6, and an uncapped mesh could keep a launch running for minutes)
 *   planes [][4]        one row per face (coplanar triangles joined): unit outward normal | offset, n . x <= o inside
 *   edges [][4]         the two end vertices and the two faces that meet at the edge, numbered within the hull
 *   pairs [npairs][2]   indices into the HULL list; a pair's first hull stays in registers while it does not change
 * A second call replaces the set; nhulls = 0 clears it.  FBR_E_INVALID: counts above the limits, an index out of range, a hull paired with
 * itself, a pair of two world hulls, a world hull without rot, non-finite data, a normal that is not unit to 1e-9, a vertex outside one of
 * its hull's planes by more than 1e-9 x the hull's diameter, an edge whose two faces are the same; the set in place before a refused call stays.
 */
#define FBR_MAX_HULLS 4096
#define FBR_MAX_HULL_PAIRS 262144
#define FBR_MAX_HULL_VERTICES 128   /* per hull, fbr_model_set_hulls: bounds the edge-pair loop that ONE LANE walks for a touching pair
                                     * (E_A E_B <= 378^2 arc tests).  Larger hulls: fbr_model_set_large_hulls below */
int fbr_model_set_hulls(fbr_model *m, int32_t nhulls, const int32_t *link, const double *offset, const double *rot,
                        int32_t offset_in_link_axes, const int32_t *vbeg, const double *verts, const int32_t *fbeg,
                        const double *planes, const int32_t *ebeg, const int32_t *edges, int32_t npairs, const int32_t *pairs);

/*
 * The same set with hulls of up to FBR_MAX_LARGE_HULL_VERTICES vertices: the hulls of visual meshes (KUKA LWR4 has no collision meshes; its
 * eight hulls have 158 to 793 vertices).  Arguments, checks and rules of fbr_model_set_hulls, which keeps refusing 129 vertices; the call
 * replaces the hull set in place, whichever of the two calls installed it, and either call replaces a set this one installed.
 * fbr_candidate_hull_distances serves such a set pair by pair: a pair whose two hulls both have at most FBR_MAX_HULL_VERTICES vertices goes
 * to the kernel of fbr_model_set_hulls and returns the bits it returns from that call; every other pair goes to
 * fbr_hull_large_pairs_kernel (csrc/fbr_hull_large.h), where the 64 lanes of a wave share the facet pass of a touching sample -- the same
 * value (the maximum over the same facets; the sign of a zero gap may differ), the same bits on every run.  Option "hull_large_all" = 1
 * sends every pair of a set installed by THIS call to that kernel (not while triangle meshes are attached to it, which needs a set
 * of small hulls only: then fbr_model_set_hull_meshes' split of the pairs holds).
 * While a hull of the set has more than FBR_MAX_HULL_VERTICES vertices, fbr_model_set_hull_meshes, fbr_hull_distance_gradients and
 * fbr_mesh_distance_gradients return FBR_E_INVALID with the hull's number and its vertex count in the message: meshes on large hulls are
 * not built, and the gradients of such a set have an entry point of their own, fbr_large_hull_distance_gradients below.  The option
 * "hull_large_all" applies to that call as well.
 */
#define FBR_MAX_LARGE_HULL_VERTICES 1024   /* per hull, fbr_model_set_large_hulls: E_A E_B <= 3066^2 arc tests, shared by 64 lanes */
int fbr_model_set_large_hulls(fbr_model *m, int32_t nhulls, const int32_t *link, const double *offset, const double *rot,
                              int32_t offset_in_link_axes, const int32_t *vbeg, const double *verts, const int32_t *fbeg,
                              const double *planes, const int32_t *ebeg, const int32_t *edges, int32_t npairs, const int32_t *pairs);

/*
 * Per candidate and hull pair the smallest signed distance over the checked samples and the sample where it is reached: arguments, outputs
 * and rules of fbr_candidate_box_distances (strict < from 1e10, the first sample wins a tie, a NaN never wins, 1e10 / -1 when no sample
 * wins, no atomics: the same bits on every run).  Separated hulls: the Euclidean distance (GJK, exact to rounding); touching or
 * overlapping: minus the minimum translation that separates them.  The reference's FCL returns a GJK/EPA value of tolerance 1e-6, build-
 * dependent when negative: the sign agrees.
 * FBR_E_INVALID: no hull set or one without pairs, ncand < 1, step < 1, num_samples 0 or not a multiple of ncand.
 */
int fbr_candidate_hull_distances(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, int32_t step,
                                 double *dist_out, int64_t *idx_out, int32_t out_mem);

/*
 * Triangle meshes on hulls of the set fbr_model_set_hulls put in place: the reference's fullMeshLinks and collisionMode "full", in which a
 * link's geometry is the triangle mesh itself (an FCL BVH) instead of its convex hull -- cages and other concave shapes.  Host arrays,
 * copied; the triangles of mesh i are rows [tbeg[i], tbeg[i + 1]) of tris:
 *   hull [nmesh]        the hull (index into the hull list) that carries mesh i; its hull stays in the hull tables
 *   tbeg [nmesh + 1]    starts at 0, ascending
 *   tris [][9]          three vertices a triangle, in the hull's axes; winding is irrelevant, zero-area triangles are kept
 * With meshes attached, fbr_candidate_hull_distances serves every pair with a mesh on either side by the mesh routine: the distance of a
 * mesh to the other hull (a solid), or to the other mesh, is the minimum over its triangles (triangle pairs) of the Euclidean distance,
 * and EXACTLY 0.0 where they touch or intersect -- never negative; a geometry wholly inside a closed mesh that does not touch its surface
 * has a positive distance (FCL's BVH behaves the same way).  Pairs without a mesh return the bits they return without any mesh attached.
 * Brute force over the triangles, culled by bounding spheres without changing a bit (csrc/fbr_mesh.h); the two limits keep a launch from
 * running for minutes: they admit every pair of the WALK-MAN simple/ collision meshes (170 x 160 = 27 200) and refuse visual meshes.
 * nmesh = 0 clears the attachments, and so does every later fbr_model_set_hulls.  fbr_hull_distance_gradients returns FBR_E_UNSUPPORTED
 * while meshes are attached: fbr_mesh_distance_gradients serves such a set.  FBR_E_INVALID: no hull set, a hull index out of range or given twice, a world hull (the reference never
 * meshes world links), tbeg not starting at 0 or not ascending, a mesh with no triangle, non-finite data, a triangle vertex outside one
 * of its hull's planes by more than 1e-9 x the hull's diameter (the culling sphere of a hull is taken over its vertices and its mesh's), a mesh
 * of more than FBR_MAX_MESH_TRIANGLES triangles, a pair of the set with T_A x T_B above FBR_MAX_MESH_PAIR_WORK; the attachments in place
 * before a refused call stay, and so they do when the call fails for another reason (an allocation).
 */
#define FBR_MAX_MESH_TRIANGLES 256
#define FBR_MAX_MESH_PAIR_WORK 32768
int fbr_model_set_hull_meshes(fbr_model *m, int32_t nmesh, const int32_t *hull, const int32_t *tbeg, const double *tris);

/*
 * The same attachment for meshes of up to FBR_MAX_LARGE_MESH_TRIANGLES triangles, on a hull set of fbr_model_set_hulls OR of
 * fbr_model_set_large_hulls: the visual meshes of KUKA LWR4 (1098 to 4434 triangles on hulls of 158 to 793 vertices), collisionMode "full"
 * on robots without collision meshes.  Arguments, attachment rules (in place; nmesh = 0 clears; a later fbr_model_set_hulls /
 * fbr_model_set_large_hulls clears; a refused or failed call leaves what was there) and every check as for fbr_model_set_hull_meshes, but
 * for the cap on the triangles of a mesh, and no cap on a pair's T_A x T_B: at set time a bounding-sphere tree is built per mesh (median
 * splits, leaves of 8 triangles; the triangles are reordered inside the library), and fbr_candidate_hull_distances sends every pair with a
 * meshed hull to a kernel that walks the two trees for the 64 samples of a wave together (csrc/fbr_mesh_bvh.h).  The value is the one
 * fbr_model_set_hull_meshes defines -- the minimum over triangles (triangle pairs), exactly 0.0 on contact, never negative -- with the
 * bits the brute force gives on the same poses: the tree only skips what could not have won.  Pairs without a mesh go to the kernels
 * they go to without any mesh attached and return the same bytes.  The gradients of such a set have an entry point of their own,
 * fbr_large_mesh_distance_gradients below: fbr_hull_distance_gradients, fbr_mesh_distance_gradients and fbr_large_hull_distance_gradients
 * return FBR_E_UNSUPPORTED while such attachments are in place.
 * FBR_E_INVALID in addition: a tree deeper than the traversal's stack holds (median splits of 8192 triangles cannot produce one).
 */
#define FBR_MAX_LARGE_MESH_TRIANGLES 8192
int fbr_model_set_large_hull_meshes(fbr_model *m, int32_t nmesh, const int32_t *hull, const int32_t *tbeg, const double *tris);

/*
 * Capsule distance and its derivative with respect to the joint positions at ONE chosen configuration per candidate and pair -- the
 * collision block of the reference's analytical gradient (excitation/analyticalGradient.py:955-1027 with capsule.py
 * capsule_distance_and_gradient), for the configurations fbr_candidate_capsule_distances found.  st, base_pos, ncand as there (ncand equal
 * candidates of T = num_samples / ncand samples; only q and base_rpy are read).  Arrays [ncand][npairs], in st->mem:
 *   sample       int64: the sample inside the candidate whose row of q is taken; -1: no evaluation (dist_out 1e10, a zero gradient row)
 *   scale        or NULL (1): the evaluated configuration is scale * q[sample] (a transition ramp s(tau) q)
 *   pose_sample  int64 or NULL (= sample; an entry -1 also means sample): the sample whose base pose (base_rpy, base_pos) is used
 * Outputs (out_mem):
 *   dist_out [ncand][npairs]       the capsule distance there: the segment routine of fbr_candidate_capsule_distances, minus the radii
 *   grad_q_out [ncand][npairs][n]  d dist / d(the evaluated configuration): n . (dp_A/dq_j - dp_B/dq_j), n the unit vector between the closest
 *                                  points p_A, p_B, each moving rigidly with its link (revolute joint j above the link: z_j x (p - o_j);
 *                                  prismatic: z_j).  Joints that are not on the tree path between the two links are exact zeros.  The
 *                                  base pose is held constant.  Multiply by scale for the derivative with respect to q[sample].
 * Zero row where |p_A - p_B| < 1e-12 (the reference's rule); a NaN pose gives NaN in dist_out and in the path joints' entries.  The
 * lever arm is v + omega x r: the reference's _point_jacobian has the opposite sign of the cross product.  No atomics:
 * the same bits on every run.
 * FBR_E_INVALID: no capsule set or one without pairs, ncand < 1, num_samples 0 or not a multiple of ncand, a sample or pose_sample outside
 * -1 .. T - 1 (found on the device, which reads such an entry clamped; the outputs are then undefined).
 */
int fbr_capsule_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                   const double *scale, const int64_t *pose_sample, double *dist_out, double *grad_q_out, int32_t out_mem);

/*
 * Signed box distance and its derivative with respect to the joint positions at ONE chosen configuration per candidate and box pair -- the
 * box pairs of the collision block of the reference's analytical gradient (excitation/analyticalGradient.py _collision_fd_single_pair: central
 * differences with analyticalGradientEpsilon), for the configurations fbr_candidate_box_distances found.  st, base_pos, ncand, sample, scale,
 * pose_sample, the memory spaces and the zeroing of grad_q_out exactly as for fbr_capsule_distance_gradients; npairs is the box set's.
 *   epsilon                        the step of the central difference (finite, positive; the reference's default 1e-7)
 *   dist_out [ncand][npairs]       the box distance of fbr_candidate_box_distances at the configuration
 *   grad_q_out [ncand][npairs][n]  (dist(q + epsilon e_j) - dist(q - epsilon e_j)) / (2 epsilon), the links below joint j moved rigidly: by
 *                                  the rotation through epsilon about the joint's world axis (revolute) or the translation along it
 *                                  (prismatic).  A robot box's centre follows center_in_link_axes (0: the offset keeps its world direction).
 *                                  Exact zeros, never evaluated: fixed joints, joints above neither link, and joints above BOTH links
 *                                  when they move the pair rigidly -- always with center_in_link_axes 1, prismatic joints with 0; with 0 a
 *                                  revolute joint above both links turns the links but not the offsets and IS evaluated.  With a world
 *                                  box every moving joint above the robot link is evaluated.  The base pose is held constant.
 * A NaN pose gives NaN in dist_out and in the path joints' entries.  No atomics: the same bits on every run.
 * FBR_E_INVALID: epsilon not finite or not positive, no box set or one without pairs, ncand < 1, num_samples 0 or not a multiple of ncand, a
 * sample or pose_sample outside -1 .. T - 1 (found on the device, which reads such an entry clamped; the outputs are then undefined).
 */
int fbr_box_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                               const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                               int32_t out_mem);

/*
 * Signed convex-hull distance and its derivative with respect to the joint positions at ONE chosen configuration per candidate and hull
 * pair -- the collision block of the reference's analytical gradient in its default collisionMode "convex" (central differences with
 * analyticalGradientEpsilon), for the configurations fbr_candidate_hull_distances found.  Arguments, memory spaces, the zeroing of grad_q_out
 * and every rule exactly as for fbr_box_distance_gradients; npairs is the hull set's.
 *   dist_out [ncand][npairs]       the hull distance of fbr_candidate_hull_distances at the configuration
 *   grad_q_out [ncand][npairs][n]  (dist(q + epsilon e_j) - dist(q - epsilon e_j)) / (2 epsilon), the links below joint j moved rigidly as for
 *                                  the boxes; a robot hull's offset follows offset_in_link_axes as a box centre follows
 *                                  center_in_link_axes, and the same entries are exact zeros, never evaluated.  A world hull never moves.
 * A NaN pose gives NaN in dist_out and in the evaluated joints' entries.  No atomics: the same bits on every run.
 * FBR_E_INVALID: epsilon not finite or not positive, no hull set or one without pairs, ncand < 1, num_samples 0 or not a multiple of ncand, a
 * sample or pose_sample outside -1 .. T - 1 (found on the device, which reads such an entry clamped; the outputs are then undefined).
 */
int fbr_hull_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                int32_t out_mem);

/*
 * The same for a hull set with triangle meshes attached (fbr_model_set_hull_meshes): the gradient half of fullMeshLinks and collisionMode
 * "full".  The reference has no rule of its own for meshes: the same central differences of whatever distance the link's geometry gives.
 * Arguments, memory spaces, the zeroing of grad_q_out and every rule exactly as for fbr_hull_distance_gradients; npairs is the hull set's,
 * ALL its pairs:
 *   a pair without a mesh   the bytes fbr_hull_distance_gradients returns for it from the same set without meshes
 *   a pair with a mesh      dist_out the mesh distance of fbr_candidate_hull_distances at the configuration, grad_q_out its central
 *                           differences, the links moved and the entries left exact zeros as for the hulls
 * A mesh distance is never negative and exactly 0.0 on contact, so an entry whose two stencil values are both 0.0 is exactly 0.0: a mesh
 * carries no penetration depth, and a pair in intersection gives the optimiser no direction out of it (FCL's BVH gives the reference the
 * same zeros).  A NaN pose gives NaN in dist_out and in the evaluated joints' entries only.  No atomics: the same bits on every run.  The
 * mesh pairs take a workspace of ncand x (stencil points of all mesh pairs) x 14 doubles (csrc/fbr_mesh_grad.h).
 * FBR_E_INVALID: what fbr_hull_distance_gradients refuses, and a set without meshes attached (that call serves it).
 */
int fbr_mesh_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                int32_t out_mem);

/*
 * fbr_hull_distance_gradients for a hull set installed by fbr_model_set_large_hulls: hulls of up to FBR_MAX_LARGE_HULL_VERTICES vertices --
 * KUKA LWR4 in the reference's default collisionMode "convex", whose hulls all have more than FBR_MAX_HULL_VERTICES vertices.  It replaces
 * the same call site: the `else` branch of the collision block of excitation/analyticalGradient.py, per joint two whole-robot forward
 * kinematics and two fcl.distance calls at q +- analyticalGradientEpsilon e_j.  Arguments, layouts, memory spaces, the zeroing of
 * grad_q_out, the exact zeros and the error rules are those of fbr_hull_distance_gradients; npairs is the hull set's.
 * A pair of two hulls of at most FBR_MAX_HULL_VERTICES vertices goes through the kernel of fbr_hull_distance_gradients and returns the bits
 * that call returns for it from a set of fbr_model_set_hulls.  Every other pair -- every pair with option "hull_large_all" = 1 -- goes
 * through three stages (csrc/fbr_hull_large_grad.h): the relative poses of the 1 + 2 J stencil points are recorded, one distance per
 * recorded pose is evaluated with the facet pass of a touching entry shared by the 64 lanes of a wave as in fbr_candidate_hull_distances,
 * and the quotients (d+ - d-) / (2 epsilon) are formed.  The values are those of the one-lane routine (a maximum over the same facets; the
 * sign of a zero gap may differ).  Option "hull_grad_tile": the live lanes of a work item of the distance stage; a value never depends on
 * it.  No atomics: the same bits on every run.
 * FBR_E_INVALID, by name: a set not installed by fbr_model_set_large_hulls, a set with no pair, epsilon not finite or not positive, option
 * "hull_grad_tile" neither 0 nor a power of two from 1 to 64; and what fbr_hull_distance_gradients refuses.  FBR_E_UNSUPPORTED: triangle
 * meshes attached (possible only while no hull of the set is above FBR_MAX_HULL_VERTICES).  fbr_hull_distance_gradients and
 * fbr_mesh_distance_gradients keep refusing a set with a hull above FBR_MAX_HULL_VERTICES vertices.
 */
int fbr_large_hull_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                      const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                      int32_t out_mem);

/*
 * The same for a hull set of fbr_model_set_hulls OR fbr_model_set_large_hulls while meshes attached by fbr_model_set_large_hull_meshes are in
 * place: the gradient half of collisionMode "full" on KUKA LWR4 (and of fullMeshLinks there).  Arguments, layouts, memory spaces, the
 * zeroing of grad_q_out, the exact zeros and the rule -- central differences over epsilon on the stencil of the other gradient calls -- are
 * those of fbr_mesh_distance_gradients; npairs is the hull set's, ALL its pairs, each through the route of its class:
 *   two hulls of at most FBR_MAX_HULL_VERTICES vertices, no mesh   the bytes fbr_hull_distance_gradients returns for the pair from a set
 *                                                                  without meshes
 *   a hull above FBR_MAX_HULL_VERTICES vertices, no mesh           the bytes fbr_large_hull_distance_gradients returns for the pair from the
 *                                                                  set without meshes (its three stages, option "hull_grad_tile")
 *   a mesh on either side                                          the stencil's relative poses are recorded and the quotients formed as by
 *                                                                  fbr_mesh_distance_gradients; in between one mesh distance per recorded
 *                                                                  pose is evaluated through the trees (csrc/fbr_mesh_bvh_grad.h)
 * A stencil value of a mesh pair has the bits the brute force over all triangle pairs gives for its pose (the traversal of
 * fbr_candidate_hull_distances, unchanged), so a set whose meshes fit both attachments returns the bytes of fbr_mesh_distance_gradients.  A
 * wave of the tree stage holds 64 consecutive entries (stencil point, candidate) of ONE mesh pair; option "mesh_grad_order" chooses their
 * order, and a value never depends on it.  Option "hull_large_all" has no effect on this call.  A mesh distance is never negative and exactly
 * 0.0 on contact: a pair in intersection has an exactly zero row.  A NaN pose gives NaN in dist_out and in the evaluated joints' entries
 * only.  No atomics: the same bits on every run.  Workspace: ncand x (stencil points of all mesh pairs and of all pairs of the second class)
 * x 14 doubles.
 * FBR_E_INVALID, by name, the set left in place: no hull set or a set with no pair; no attachment of fbr_model_set_large_hull_meshes (the
 * message names the call that serves the set: fbr_mesh_distance_gradients for small meshes, fbr_large_hull_distance_gradients for large
 * hulls without meshes, fbr_hull_distance_gradients for small hulls without meshes); epsilon not finite or not positive; option
 * "mesh_grad_order" not 0, 1 or 2; option "hull_grad_tile" as for fbr_large_hull_distance_gradients where the set has a pair of the second
 * class (it is not looked at otherwise); and the argument checks of
 * fbr_hull_distance_gradients.
 */
int fbr_large_mesh_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                      const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                      int32_t out_mem);

/*
 * tau_out [S][rows] = Y_s . x for an identified-parameter vector x (host, length cols) WITHOUT
 * materialising Y -- Identification.estimateRegressorTorques' np.dot(YStd, x) (identifier.py:135-141).
 */
int fbr_predict(fbr_model *m, const fbr_states *st, const double *x, double *tau_out, int32_t out_mem);

/*
 * out [S][rows] = J_frame^T w per sample for a frame rigidly attached to `link` at (frame_R, frame_p)
 * (host, 9 and 3 doubles); wrench [S][6] in st->mem.  getFrameFreeFloatingJacobian + J^T w
 * (model.py:542-555).  Uses st->q and st->base_rpy only.
 */
int fbr_contact_torques(fbr_model *m, const fbr_states *st, int32_t link, const double *frame_R,
                        const double *frame_p, const double *wrench, double *out, int32_t out_mem);

/* ---- fused reductions (Y is never materialised) ----------------------------------------------- */
/*
 * G_out [(cols+k)][(cols+k)] (+)= [Y | rhs]^T diag(w)^2 [Y | rhs], the raw (un-normalised) Gram of the
 * stacked regressor augmented with k right-hand-side columns rhs [S*rows][k] (tau, contact forces, ...),
 * row weights w [S*rows] optional (NULL = 1; a 0/1 mask selects e.g. the base-wrench rows of
 * identifier.py:617-681).  accumulate != 0 adds to the existing content of G_out.
 * Serves: R += A^T A of getRandomRegressor (model.py:803-806), YBase^T YBase = G[ic,ic]
 * (identifier.py:361, trajectoryOptimizer.py:263), YBase^T tau, and the OLS normal equations.
 * rhs / w live in st->mem; G_out in out_mem.
 */
int fbr_gram_accumulate(fbr_model *m, const fbr_states *st, const double *rhs, int32_t k, const double *w,
                        double *G_out, int32_t out_mem, int32_t accumulate);

/*
 * Asynchronous form of fbr_gram_accumulate for callers that keep everything in HBM (states, rhs, w and G_out device resident): the
 * pass is enqueued and the call returns; *ticket identifies it.  Up to TWO submissions are in flight (a third one first waits for
 * the oldest); the kinematics / packing of a submission's first chunk then run beside the last Gram launches of the one before --
 * the only producer work of a pass that nothing else hides (a sample loop split over several calls, model.py:370, or one rank's short
 * shard per step).  G_out must not be read, and the inputs not rewritten, before fbr_wait(m, ticket) has returned.  Every blocking
 * entry point of the same model first waits for all submissions.  fbr_wait: ticket < 0 waits for everything submitted so far.
 */
int fbr_gram_submit(fbr_model *m, const fbr_states *st, const double *rhs, int32_t k, const double *w, double *G_out,
                    int32_t accumulate, int64_t *ticket);
int fbr_wait(fbr_model *m, int64_t ticket);

/*
 * The same reduction for ngroups consecutive, equally sized groups of samples in ONE pass: G_out [ngroups][(cols+k)][(cols+k)],
 * group g = samples [g*S/ngroups, (g+1)*S/ngroups) (num_samples must be a multiple of ngroups).  Serves the
 * trajectory optimiser's inner loop (excitation/trajectoryOptimizer.py:248-272: YBase^T YBase of every candidate
 * trajectory) and finite-difference sweeps, where one Gram per small trajectory would be launch-bound.
 */
int fbr_gram_grouped(fbr_model *m, const fbr_states *st, int32_t ngroups, const double *rhs, int32_t k, const double *w,
                     double *G_out, int32_t out_mem);

/*
 * Finite-difference sweep of a weighted regressor score (the per-sample worker of the analytical trajectory gradient,
 * excitation/analyticalGradient.py:92-185): out [num_samples][1 + 3 n] with
 *   out[s][0]        = sum_{r,c} W_s[r][c] * Y_s[r][c]                     (baseline state of sample s)
 *   out[s][1 + d]    = the same sum for the state with q_d   + eps,
 *   out[s][1+n + d]  =                                    dq_d  + eps,
 *   out[s][1+2n + d] =                                    ddq_d + eps      (d = 0..n-1),
 * W [num_samples*rows][cols] the weight blocks (st->mem).  (out[s][1+j] - out[s][0]) / eps are the reference's
 * sens_q / sens_dq / sens_ddq; the 1 + 3 n regressor blocks per sample are evaluated on the fly, never stored.
 */
int fbr_fd_scores(fbr_model *m, const fbr_states *st, const double *W, double eps, double *out, int32_t out_mem);

/*
 * Weight rows of the D-optimality gradient, formed on the device: W [S][rows][P] (P = every column of the model, friction columns
 * included: the layout fbr_fd_scores reads) with
 *   W[s][:, cols] = Y_s[:, cols] . C[g(s)],   g(s) = s / (S / ngroups),   every column not in cols = exact 0.0 (whatever W held before).
 * The reference builds them on the host for ONE trajectory -- R_dopt = -2 scale YBase (YBase^T YBase + delta I)^-1 by SVD or solve and
 * W_std = R_dopt Pb^T over the stacked regressor (excitation/analyticalGradient.py:538-565, W_iner / W_visc 578-596); with YBase =
 * Y[:, cols] Pb that is Y[:, cols] times a constant ncols x ncols matrix per candidate, C = -2 scale Pb (Pb^T G Pb + delta I)^-1 Pb^T.
 *   cols [ncols] (host; no repeats, any order) or NULL: every column (ncols is then ignored);  C [ngroups][ncols][ncols] row-major,
 *   general (no symmetry assumed), in st->mem space like the states;  W in `mem` space.  The regressor kernel of fbr_regressor_batch writes
 *   Y into W and an fp64 MFMA kernel transforms it in place, row tile by row tile (csrc/fbr_weights.h); no atomics, the same bits on every
 *   run and for every chunking.
 * num_samples == 0 is a no-op.  FBR_E_INVALID: num_samples not a multiple of ngroups, ngroups < 1, a bad column list;
 * FBR_E_UNSUPPORTED: more than 1196 selected columns (a 16-row tile has to fit the LDS).
 */
int fbr_regressor_weights(fbr_model *m, const fbr_states *st, int32_t ngroups, const int32_t *cols, int32_t ncols, const double *C, double *W,
                          int32_t mem);

/*
 * The D-optimality arithmetic of ngroups candidates from their Grams G [ngroups][Pa][Pa] (fbr_gram_grouped), on the device: per candidate c
 *   M_c = G_c[cols, cols] (+ prior),  only its LOWER triangle is read (what numpy.linalg.eigvalsh reads),
 *   eig_c: the eigenvalues of M_c, ascending (Householder tridiagonalisation, bisection on Sturm counts: absolute error of order
 *          eps |M_c|, LAPACK's error model; M_c is first scaled by a power of two, so the spectrum of 2^k G is exactly 2^k times that of G),
 *   terms[c] = { neg_log_det = -sum_i log(max(eig_i + delta, 1e-300)),  lambda_max = eig_{n-1},  delta = reg max(lambda_max, 1e-30),
 *                n_observable = #(eig_i > delta) }       (excitation/trajectoryOptimizer.py:263-277),
 *   Cmat[c] = -2 scale[c] (M_c + delta I)^-1, exactly symmetric (Cholesky; analyticalGradient.py:538-565): the C of fbr_regressor_weights.
 * cols [ncols]: host, distinct, any order, 0 <= col < Pa;  prior [ncols][ncols] in `mem` space like G, or NULL;  scale [ngroups]: host, or
 * NULL (= 1);  terms [ngroups][4], status [ngroups] or NULL, eig [ngroups][ncols] or NULL, Cmat [ngroups][ncols][ncols] or NULL: `mem` space.
 * status[c]: 0, or bit 1 (value 1): M_c has a non-finite entry -- the candidate's terms, eig and Cmat are NaN, n_observable 0 --, bit 2
 * (value 2): a pivot of the factorisation was not positive (reg = 0 on a singular matrix): Cmat[c] is NaN, its terms stand.  One
 * candidate's outputs depend on nothing but that candidate: no atomics, fixed summation orders, the same bits on every run, in both
 * memory spaces and with or without eig / Cmat.  One workgroup per candidate, chunks of at most 65535 candidates (csrc/fbr_dopt.h).
 * FBR_E_INVALID: ngroups < 1, ncols outside 1 .. min(Pa, FBR_MAX_DOPT_COLUMNS), an index out of range or twice, reg negative or not finite.
 */
#define FBR_MAX_DOPT_COLUMNS 512
int fbr_dopt_terms(fbr_model *m, const double *G, int32_t ngroups, int32_t Pa, const int32_t *cols, int32_t ncols, const double *prior, double reg,
                   const double *scale, double *terms, int32_t *status, double *eig, double *Cmat, int32_t mem);

/*
 * The observability analysis of ngroups candidates from their Grams, on the device: what the reference runs on YBase of the chosen
 * trajectory by SVD (trajectory.py:225-264), here per candidate on M_c = G_c[cols, cols] (+ prior) of fbr_dopt_terms, whose eigenvalues
 * are S^2 and whose eigenvectors are the right singular vectors of YBase:
 *   eig_c: bit for bit the eigenvalues fbr_dopt_terms reports;  vec[c][j][i]: component j of the eigenvector of eig[c][i] (the kept
 *          Householder reflectors, implicit QL with Wilkinson shifts; residual and orthogonality of order n eps |M_c|, also inside
 *          clusters such as the null space of unexcited joints); its component of largest magnitude, the first at a tie, is positive;
 *   lm = max(eig_max, 0), cut = threshold^2 lm;  index i is unobservable iff max(eig_i, 0) < cut (S_i < threshold S_0: for the zero matrix
 *          nothing is);  n_observable[c] = ncols - their number;  energy[c][j] = sum over the unobservable i, ascending, of vec[c][j][i]^2;
 *   margin[c] = min_i |eig_i - cut| / cut (+inf when cut = 0).
 * The limit of the Gram route: fp64 knows an eigenvalue of M_c to about band lm, band(ncols) = max(128, ncols) 2^-52, hence a singular
 * value of YBase only down to about 2e-7 S_0.  FBR_E_INVALID for a threshold outside (0, 1) or with threshold^2 < 8 band (1e-6, the
 * reference's default, passes up to ncols = 512); status bit 4 (value 4) where some eig_i lies within band lm of the cut: the
 * classification of that index is not decided by this arithmetic, the numbers are returned all the same.  Agreement with an SVD of YBase
 * for singular values between 1e-8 S_0 and the threshold is a property of the Gram, not of the kernel.
 * cols, prior: as for fbr_dopt_terms.  n_observable [ngroups], energy [ngroups][ncols], margin [ngroups] or NULL, eig [ngroups][ncols] or
 * NULL, vec [ngroups][ncols][ncols] or NULL, status [ngroups] or NULL: `mem` space.  status[c]: bit 1 (value 1): a non-finite entry -- the
 * candidate's outputs are NaN, n_observable 0 --; bit 4: above; bit 8 (value 8): the QL iteration used up its 30 ncols sweeps -- vec and
 * energy of that candidate are NaN, the rest stands.  One candidate's outputs depend on nothing but that candidate; the same bits on every
 * run, in both memory spaces and with or without margin / eig / vec.  One workgroup per candidate, 2 ncols^2 doubles of scratch each.
 * FBR_E_INVALID also for what fbr_dopt_terms refuses.
 */
int fbr_dopt_observability(fbr_model *m, const double *G, int32_t ngroups, int32_t Pa, const int32_t *cols, int32_t ncols, const double *prior,
                           double threshold, int32_t *n_observable, double *energy, double *margin, double *eig, double *vec, int32_t *status,
                           int32_t mem);

/*
 * Joint states of ncand candidate trajectories, T samples each, generated ON THE DEVICE from their Fourier coefficients -- the
 * parametrisation the trajectory optimiser searches over (excitation/trajectoryGenerator.py: OscillationGenerator 411-460,
 * BoundedOscillationGenerator 462-560; evaluated per candidate by computeTrajectoryDynamics 83-128 before every objective call,
 * trajectoryOptimizer.py:240-272).  q / dq / ddq [ncand * T][n] (out_mem space) are laid out like fbr_states of ncand groups, i.e. ready
 * for fbr_gram_grouped: a candidate crosses PCIe as 2 n nharm + n + 1 coefficients instead of 3 n T samples.
 *   wf [ncand], a / b [ncand][n][nharm] (harmonics beyond a joint's own nf: 0), q_offset [ncand][n], q_range [ncand][n] or NULL: host arrays.
 *   q_range == NULL (classic, Swevers 1997):  dq = sum_l a_l cos(wf l t) + b_l sin(wf l t), q its integral + q_offset (= nf q0), ddq its derivative
 *   q_range != NULL (bounded):                 q = q_offset + q_range tanh(sum_l a_l sin(wf l t) + b_l cos(wf l t)) (q_offset = q_center), dq, ddq by the chain rule
 * t = sample index / freq (radians; useDeg of the reference converts on the host before / after).
 */
int fbr_fourier_states(fbr_model *m, int32_t ncand, int64_t T, int32_t nharm, double freq, const double *wf, const double *a, const double *b,
                       const double *q_offset, const double *q_range, double *q, double *dq, double *ddq, int32_t out_mem);

/*
 * Chain of per-sample sensitivities with the Jacobian of the series fbr_fourier_states evaluates -- Phase B of the reference's analytical
 * gradient (excitation/analyticalGradient.py:664-762: Python loops over joints and harmonics; its wf column, line 672, from central
 * differences of the whole trajectory, _compute_wf_derivatives) for ncand candidates in one call.  sens_q / sens_dq / sens_ddq
 * [ncand * T][n] (sens_mem space): the sensitivities of sample i = 0 .. T - 1 of every candidate, taken at time i * tstride / freq
 * (tstride > 1: the sub-sampled sweep of analyticalGradientSubsample).  wf, a, b, q_range: host arrays as for fbr_fourier_states.
 *   out [ncand][1 + 2 n + 2 n nharm] (out_mem) = [d/dwf | d/dq_offset (n) | d/dq_range (n; zeros when q_range == NULL) | d/da (n, nharm) |
 *   d/db (n, nharm)],  each entry = sum_t sum_j sens_q dq/dp + sens_dq d(dq)/dp + sens_ddq d(ddq)/dp, every derivative analytic (wf too).
 * Harmonics beyond a joint's own nf (coefficient 0) are differentiated like the others: the caller drops them.  Fixed summation order
 * (per-block partials, then a finishing pass): the same bits on every run.
 */
int fbr_fourier_gradient(fbr_model *m, int32_t ncand, int64_t T, int32_t tstride, int32_t nharm, double freq, const double *wf, const double *a,
                         const double *b, const double *q_range, const double *sens_q, const double *sens_dq, const double *sens_ddq,
                         int32_t sens_mem, double *out, int32_t out_mem);

/*
 * Chain of rows of position sensitivities, each taken at ONE time, with the position Jacobian of the same series: nrows rows per candidate
 * (the collision pairs of fbr_capsule_distance_gradients), sample / scale [ncand][nrows] and grad_q [ncand][nrows][n] in `mem` space
 * (sample int64; scale may be NULL: 1); wf, a, b, q_range host arrays as for fbr_fourier_gradient.
 *   out [ncand][nrows][1 + 2 n + 2 n nharm] (out_mem), the column layout and conventions of fbr_fourier_gradient (padding harmonics
 *   differentiated too, the q_range columns zero when q_range == NULL):  entry = scale * sum_d grad_q[d] * dq_d/dp at t = sample / freq,
 *   every derivative analytic (wf too).  A row with sample < 0 is zero.  The wf entry adds its joints in ascending order: the same bits on
 *   every run.
 */
int fbr_fourier_position_chain(fbr_model *m, int32_t ncand, int64_t nrows, int32_t nharm, double freq, const double *wf, const double *a,
                               const double *b, const double *q_range, const int64_t *sample, const double *scale, const double *grad_q,
                               int32_t mem, double *out, int32_t out_mem);

/*
 * The same chain for rows that carry sensitivities to the joint velocities and accelerations as well -- the torque, position and velocity
 * rows of the constraint Jacobian and of the soft-cost gradients (analyticalGradient.py:764-953, there a Python loop per row over joints
 * and harmonics).  grad_q / grad_dq / grad_ddq [ncand][nrows][n] in `mem` space, each may be NULL (zero); everything else as for
 * fbr_fourier_position_chain.
 *   out [ncand][nrows][1 + 2 n + 2 n nharm]:  entry = scale * sum_d (grad_q[d] dq_d/dp + grad_dq[d] d(dq_d)/dp + grad_ddq[d] d(ddq_d)/dp)
 *   at t = sample / freq, every derivative analytic (wf too: the reference takes central differences of the whole trajectory there).  A
 *   row with sample < 0 is zero; exact-zero entries of the grad arrays cost nothing; the wf entry adds its joints in ascending order.
 *   With grad_dq == grad_ddq == NULL every entry equals fbr_fourier_position_chain's (the same expression; an entry that is zero may carry
 *   the other sign).
 */
int fbr_fourier_state_chain(fbr_model *m, int32_t ncand, int64_t nrows, int32_t nharm, double freq, const double *wf, const double *a,
                            const double *b, const double *q_range, const int64_t *sample, const double *scale, const double *grad_q,
                            const double *grad_dq, const double *grad_ddq, int32_t mem, double *out, int32_t out_mem);

/*
 * R_out [(cols+k)][(cols+k)] upper triangular with R^T R = [Y|rhs]^T [Y|rhs], by blocked Householder
 * TSQR over sample blocks (no Gram squaring of the condition number; on branched robots the rows are grouped along
 * the kinematic tree and every group is factorised over the columns it can touch -- same R).  If R_in != NULL it is an
 * existing triangular factor (same shape, out_mem space) that is folded in first (streaming / tree
 * reduction across calls and ranks).  Serves la.qr(YBase) (sdp.py:470), sla.qr(YStd, pivoting) column
 * norms / pivots (model.py:841) and lstsq (identifier.py:712) through the small host problems.
 */
int fbr_tsqr(fbr_model *m, const fbr_states *st, const double *rhs, int32_t k, const double *w,
             const double *R_in, double *R_out, int32_t out_mem);

/*
 * Same as fbr_tsqr for a COLUMN SUBSET of the regressor: R_out [(ncols+k)][(ncols+k)] with
 * R^T R = [Y[:, cols] | rhs]^T [Y[:, cols] | rhs].  cols (host, int32, ncols entries, any order, no repeats) are
 * typically Model.independent_cols, which makes this la.qr(YBase) of sdp.py:470 / the lstsq of identifier.py:712
 * at (nb+k)^2 instead of (P+k)^2 cost.  R_in, if given, is a factor of the same subset.
 */
int fbr_tsqr_cols(fbr_model *m, const fbr_states *st, const int32_t *cols, int32_t ncols, const double *rhs, int32_t k,
                  const double *w, const double *R_in, double *R_out, int32_t out_mem);

/*
 * Asynchronous form of fbr_tsqr / fbr_tsqr_cols (cols == NULL: every identified column) for callers that keep everything in HBM: the
 * factorisation is enqueued and the call returns; *ticket identifies it, fbr_wait(m, ticket) completes it (tickets are shared with
 * fbr_gram_submit: at most TWO submissions of either kind are in flight, a third one first waits for the oldest).  When the submission
 * before is a TSQR as well, the kinematics and the first chunk's regressor writer of this one run beside its merge trees -- the part of
 * a call that executes no MFMA and that the (latency-bound, few-workgroup) trees leave the CUs free for: a streamed sequence of calls
 * (la.qr of a regressor that arrives in pieces, sdp.py:470-487 over several measurement files; one rank's shard per step) pays the
 * trees once.  R_out must not be read, and the inputs / R_in not rewritten, before fbr_wait has returned; a pipeline error of the
 * kernels is reported by fbr_wait.  Row weights w are scanned for switched-off rows on the host: with w != NULL the call first waits
 * for the stream (correct, not overlapped).
 */
int fbr_tsqr_submit(fbr_model *m, const fbr_states *st, const int32_t *cols, int32_t ncols, const double *rhs, int32_t k,
                    const double *w, const double *R_in, double *R_out, int64_t *ticket);

/* R_out = R factor of [R_a; R_b] (both n x n upper triangular, row-major) -- one node of the TSQR tree. */
int fbr_tsqr_merge(fbr_model *m, int32_t n, const double *R_a, const double *R_b, double *R_out, int32_t mem);

/* ---- the step before the path: signal conditioning of measurement channels ---------------------------- */
/*
 * The array operations of Data.preprocess (identification/data.py:369-619) on channel arrays X [S][ld] (row-major, the first ncols
 * columns are processed, in place), in `mem` space; `m` only supplies the device and the stream.
 *   fbr_filtfilt      scipy.signal.filtfilt(b, a, X, axis=0) with its defaults (odd extension of 3*ncoef samples, steady-state
 *                     initial conditions): the zero-phase Butterworth low-passes of positions / velocities / torques / IMU / FT
 *                     channels (data.py:430-436, 470-480, 505-520, 600-615).  ncoef = order + 1 <= 12, S > 3*ncoef.
 *   fbr_medfilt       scipy.signal.medfilt(X, (k, 1)) (zero padding at the ends), k odd <= 31 (data.py:466, 485, 500, 598).
 *   fbr_central_diff  D [S][ncols] = 4th-order central difference of A [S][ncols] (dense) over the time stamps T [S] with the
 *                     reference's edge rules (data.py:396-418).  S >= 5.
 */
int fbr_filtfilt(fbr_model *m, const double *b, const double *a, int32_t ncoef, double *X, int64_t S, int32_t ncols, int32_t ld, int32_t mem);
int fbr_medfilt(fbr_model *m, int32_t k, double *X, int64_t S, int32_t ncols, int32_t ld, int32_t mem);
int fbr_central_diff(fbr_model *m, const double *A, const double *T, double *D, int64_t S, int32_t ncols, int32_t mem);

/* ---- profiling ---------------------------------------------------------------------------------- */
#define FBR_PROF_KIN 0       /* link kinematics kernel */
#define FBR_PROF_REGRESSOR 1 /* materialising regressor kernel */
#define FBR_PROF_GRAM 2      /* fused regressor->Gram MFMA kernel; the in-place weight GEMM of fbr_regressor_weights (its writer: REGRESSOR) */
#define FBR_PROF_REDUCE 3    /* slice reduction / scatter of the Gram partials; chain kernel + finishing pass of fbr_fourier_gradient;
                                stage B of fbr_mesh_distance_gradients by itself (the whole call, stage B included, is under KIN) */
#define FBR_PROF_ID 4        /* inverse dynamics / predict kernel */
#define FBR_PROF_TSQR 5      /* TSQR fold kernels (level 0 per chunk, merge tree) */
#define FBR_PROF_PACK 6      /* tile-image packing kernel of the fused Gram pass (producer stream) */
#define FBR_PROF_H2D 7       /* host -> device staging copies of the chunked fused pass (pinned host inputs) */
#define FBR_PROF_TREE 8      /* TSQR merge tree of the main row group on the call's stream (the latency-bound tail of a call; the other
                                groups' trees run beside it on side streams and are not counted) */
#define FBR_PROF_COUNT 9
/* When enabled, every kernel launch is bracketed by hipEvents on the launch stream; fbr_profile_get
   returns, per kernel class, the summed device time in ms and the launch count since the last reset
   (the counters are reset by the call).  Used by bench.py for the live roofline figures. */
int fbr_profile_enable(fbr_model *m, int32_t on);
int fbr_profile_get(fbr_model *m, double *ms_out /*[FBR_PROF_COUNT]*/, int64_t *launches_out /*[FBR_PROF_COUNT]*/);

/* ---- introspection (tests, tooling) ------------------------------------------------------------ */
/*
 * MFMA instructions (v_mfma_f64_16x16x4_f64, 2 * 16 * 16 * 4 = 2048 flop each) that fbr_tsqr / fbr_tsqr_cols executes for num_samples
 * samples and k rhs columns: the level-0 folds of the row-sorted chunks of every row group (a block is folded from the first
 * column its rows can touch) and the merge trees over the per-workgroup factors -- counted on the host from the same chunking and fold
 * rules the kernels use, so bench.py can report executed (not dense-model) flops.  cols == NULL: every identified column.
 * block_rows / n_padded (optional): rows per fold and padded factor width.
 */
int fbr_tsqr_work_info(fbr_model *m, const int32_t *cols, int32_t ncols, int32_t k, int64_t num_samples, int64_t *mfma_level0,
                       int64_t *mfma_tree, int32_t *block_rows, int32_t *n_padded);

/* Tile program of the fused Gram kernel that fbr_gram_accumulate runs for a batch of num_samples samples (< 0: a batch large enough
   for the column reductions below): counts of padded column tiles / tile pairs / MFMA k-steps per sample, so tests and bench.py can
   report executed vs algorithmic flops of the program that was actually executed. */
int fbr_gram_program_info(const fbr_model *m, int32_t k, int64_t num_samples, int32_t *num_tiles, int32_t *num_pairs,
                          int64_t *mfma_per_sample, int32_t *num_parts);

/* The sample-contiguous Gram pass (option "gram_lane", csrc/fbr_gram64.h) for the same batch: info[0] = 1 when the model qualifies and the
   option is on (device-resident inputs, k <= 2), else every entry is 0; [1] tile rows of a 64-sample block image, [2] its bytes, [3] MFMA
   instructions per block, [4] row levels, [5] slabs of the widest stage, [6] LDS bytes of the Gram kernel, [7] column tiles, [8] force
   tiles (option "gram_force_tiles"), [9] sum over the levels of the busiest wave's active tile pairs, [10] the same for a perfect split
   over the 8 waves, [11] stages (barriers) per half block.  The image is written once and read once per pass: 2 * info[2] / 64 bytes of HBM traffic per sample.
   Limits (info[0] = 0 beyond them, and the call takes the per-sample-image pass or the Gram from the TSQR factor): joint paths of at most
   24 joints (the one-lane-per-sample kinematics), at most 60 regressor rows, and a producer whose staged states, row weights and rhs of a
   64-sample block fit a workgroup's 160 KiB of LDS.  A pass cuts its samples into chunks whose images stay below 3 GB (also when the
   option "chunk_samples" asks for more).
   Size limits of the other entry points: fbr_predict / fbr_inverse_dynamics_batch / fbr_contact_torques run the one-kernel form for joint
   paths of at most 24 joints and at most 105 DOF (the states of 64 samples in the LDS) and the two-kernel form beyond; the fused Gram of
   fbr_gram_grouped / fbr_gram_submit takes at most 60 regressor rows; fbr_tsqr and the Gram from its factor (fbr_gram_accumulate beyond 60
   rows) at most 768 columns including the rhs.  Beyond a limit a call fails with FBR_E_UNSUPPORTED and an error text that names it. */
int fbr_gram_lane_info(const fbr_model *m, int32_t k, int64_t num_samples, int64_t info[12]);

/*
 * Column reductions (options "link_merge" / "regroup" / "reduce_min_work" below).  The regressor columns of a link attached by a FIXED
 * joint are an exact, constant linear combination of the columns of the moving body it rides on (the 10 x 10 change of frame of the
 * inertial parameters), and three parameter directions of a link behind a revolute joint act like parameters of its parent.
 * fbr_gram_accumulate / fbr_gram_submit / fbr_tsqr / fbr_tsqr_submit therefore reduce over a full-rank subset of the columns where that
 * pays and expand the small result with a constant matrix E: G = E^T G_red E, R = qr([R_in ; R_red E]) -- the same G and the same R^T R
 * to rounding (1e-15 relative), same layout, same arguments.  moving_links / reduced_cols: what a Gram pass over num_samples samples
 * runs on (< 0: a batch large enough for the reductions; == the model's own counts when nothing is reduced).
 */
int fbr_model_link_merge_info(const fbr_model *m, int64_t num_samples, int32_t *moving_links, int32_t *reduced_cols);

/* The per-sample records fbr_suspended_base_motion steps through (tests, tooling): rec_out [num_samples][39] (out_mem) = composite inertia
   about the attachment origin O (xx xy xz yy yz zz) | Coriolis coupling B (3 x 3 row-major) | joint-motion moment c0 | first mass moment mc |
   pose R (3 x 3) | p and twist [lin; ang] of the base link relative to the attachment frame; everything in the attachment link's axes.
   Arguments and errors as there. */
int fbr_suspended_records(fbr_model *m, const fbr_states *st, const double *x_std, int32_t num_x, int32_t att_link, double *rec_out,
                          int32_t out_mem);

/* ---- options ------------------------------------------------------------------------------------ */
/*
 * Per-model switches and thresholds.  The library never reads the process environment: what a call does is decided by its arguments
 * and by these options.  Setting an option first waits for every submission in flight; unknown keys fail with FBR_E_INVALID.
 *   "link_merge"                 1     column reductions on (0: every reduction runs over all columns of the model)
 *   "regroup"                    1     ... including the revolute regrouping (0: fixed links merged only)
 *   "reduce_min_work"            1e9   a Gram call takes the reductions when S (P - P_red) P >= this, a factorisation from an eighth of
 *                                      it on (0: always; the reduced pass costs a second model's launches and the expansion kernels)
 *   "reduce_grouped_min_samples" 512   fbr_gram_grouped takes them for groups of at least this many samples
 *   "chunk_samples"              0     > 0: samples per chunk of every pass (0: sized by memory)
 *   "min_chunks"                 4     a short fused pass is still cut into this many chunks
 *   "h2d_chunked"                1     pinned host inputs staged chunk by chunk on a copy stream, overlapped with the kernels
 *   "fused_id"                   1     fbr_predict / fbr_inverse_dynamics_batch run kinematics and torques in ONE kernel, the link records
 *                                      stay in registers (0: kinematics kernel + torque kernel with the records staged through HBM)
 *   "gram_lane"                  1     fused Gram over SAMPLE-contiguous images (MFMA k-steps over four samples of one regressor row) with a
 *                                      one-lane-per-sample producer, where the call allows: at most two rhs columns, a tile program in one part
 *                                      (friction columns included); inputs resident in HBM, pageable or pinned (staged chunk by chunk);
 *                                      fbr_gram_grouped without rhs columns (0: always the per-sample images of the kinematics + packer kernels)
 *   "gram_lane_waves"            8     gram_lane, models whose tile pairs need the one-workgroup-per-CU shape: workgroups of 8 waves with 18
 *                                      accumulators each (two waves per SIMD); 16: 16 waves with 10 accumulators (four per SIMD at 128
 *                                      registers: measured 4 % slower on WALK-MAN)
 *   "gram_force_tiles"           1     gram_lane: the three force rows of the base wrench run on tiles of their own that hold only the columns
 *                                      with a force (mass, first moments), when the extra tile pairs fit the accumulators (0: every tile pair
 *                                      pays the three levels)
 *   "gram_lane_tiling"           1     gram_lane: column tiles of its own for the pass (a bottom-up fill: a column may sit in any tile whose
 *                                      joint path contains its own), kept when they need fewer MFMAs than the tile program's (0: the tile
 *                                      program's tiles and pairs)
 *   "gram_lane_skip_unowned"     1     gram_lane producer: a wave forms no column of a link it walks only as an ancestor of its own links
 *                                      (0: formed and not stored); same bits
 *   "gram_lane_parts_cut"        0     gram_lane producer: 1: the tree is cut for its four waves so that the slowest one, ancestors included,
 *                                      is as fast as an instruction-count model allows (0: parts of equal owned cost); same bits; measured
 *                                      0.13 ms slower per 1 M WALK-MAN samples
 *   "gram_lane_chunk_rounds"     0     gram_lane, device-resident inputs that need several chunks: 1: chunk sizes with the fewest rounds of
 *                                      the Gram grid, then of the producer grid, then the fewest chunks (0: chunks as large as memory
 *                                      allows); measured no faster
 *   "gram_shape"                0     fused Gram kernel shape: 0 by model, 1 one workgroup per CU, 2 two per CU
 *   "gram_rhs_tile"              0     1: dense tiles for the rhs columns even for k <= 2 (default: their products come from the packer)
 *   "gram_orient"                1     tile pairs turned so that the row segments fill up
 *   "tsqr_groups"                1     rows grouped along the kinematic tree ...
 *   "tsqr_group_min_samples"     24000 ... from this many samples on
 *   "tsqr_reorder"               1     columns factorised in link-depth order (single-factorisation path)
 *   "tsqr_narrow"                1     wave-private kernels for <= 128 columns
 *   "tsqr_narrow_tall"           1     ... whose level-0 folds take 96-row blocks at one wave per SIMD for long calls over <= 6 column tiles
 *                                      (0: 48-row blocks, two waves per SIMD)
 *   "tsqr_lane_writer"           1     regressor writer of the TSQR: one lane per sample with the kinematics fused in (no records in HBM), chunks
 *                                      written column-major in 512-byte runs (0: kinematics kernel + the workgroup-per-sample writers below)
 *   "tsqr_force_group"           1     row groups of a floating base: the three FORCE rows of the base wrench form a group of their own, factorised
 *                                      over the columns that produce a force (a link's mass and first moments); the dense group keeps the three
 *                                      moment rows (0: one dense group of six rows)
 *   "tsqr_writer"                0     grouped regressor writer: 0 by work-item count; 8 / 16: one thread per column / column pair, stores of that
 *                                      width; 32: rows staged in the LDS and streamed out in 16-byte pieces (measured: no faster)
 *   "tsqr_tree_one_wg"           0     merges by one workgroup instead of pipelined across workgroups (bit-identical, slower)
 *   "tsqr_side_trees_beside"     0     row-group TSQR: 1 starts the side groups' merge trees beside the main group's last level-0 fold (the
 *                                      default of rounds 3 - 5); 0 behind it (round 6: with the force rows in a group of their own the main
 *                                      fold is half as long and a 125 k-sample call is 0.45 ms shorter this way)
 *   "tsqr_prologue_overlap"      1     a submission's kinematics / first writer beside the merge trees of the one before
 *   "tsqr_short_call_factors"    1     fewer private factors (shallower merge trees) for calls too short to amortise them
 *   "hull_large_all"             0     fbr_candidate_hull_distances, a set installed by fbr_model_set_large_hulls: 1 sends every pair to
 *                                      fbr_hull_large_pairs_kernel, also those of two hulls of at most FBR_MAX_HULL_VERTICES vertices (tests:
 *                                      the two kernels on the same pairs).  Read by every call: a later change is never ignored
 *   "hull_grad_tile"             0     fbr_large_hull_distance_gradients: the live lanes of a work item of its distance stage, a power of two from
 *                                      1 to 64 (anything else: the call returns FBR_E_INVALID); 0: the widest that leaves 12 items a CU, the waves a CU holds.  The
 *                                      touching entries of an item run their facet passes one after the other.  Read by every call
 *   "mesh_grad_order"            0     fbr_large_mesh_distance_gradients: the order of the (stencil point, candidate) entries of a mesh pair, 64
 *                                      consecutive ones a wave of its distance stage -- 1: candidate-major (a wave holds all stencil points of
 *                                      its candidates), 2: slot-major (a wave holds one stencil point of 64 candidates), 0: the default order,
 *                                      candidate-major (measured: DESIGN.md); anything else: the call returns FBR_E_INVALID.  A value never depends on it.  Read
 *                                      by every call
 *   "gram_serial", "gram_timing", "tsqr_timing"  0   diagnostics (producer on the main stream; cycle counters printed to stderr)
 * fbr_model_option_name enumerates the keys (index 0 .. until it fails).
 */
int fbr_model_set_option(fbr_model *m, const char *key, double value);
int fbr_model_get_option(const fbr_model *m, const char *key, double *value);
int fbr_model_option_name(int32_t index, const char **name);


#ifdef __cplusplus
}
#endif
#endif /* FBR_H */
