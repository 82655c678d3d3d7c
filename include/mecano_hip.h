/*
 * mecano_hip.h -- C-ABI of the MI355X batched rigid-body-dynamics engine.
 *
 * This is the drop-in boundary for ONE hot path of ihmcrobotics/mecano (Java):
 *
 *   InverseDynamicsCalculator              (RNEA)  algorithms/InverseDynamicsCalculator.java:481-501,567
 *   ForwardDynamicsCalculator              (ABA)   algorithms/ForwardDynamicsCalculator.java:475-520,556-591
 *   CompositeRigidBodyMassMatrixCalculator (CRBA)  algorithms/CompositeRigidBodyMassMatrixCalculator.java:344-348
 *
 * (paths below are relative to src/main/java/us/ihmc/mecano/ of the reference).
 *
 * The reference evaluates one configuration per compute() call, on one CPU
 * thread, reading q / qd through the MovingReferenceFrame tree.  This library
 * evaluates B configurations per call on one GPU.  A Java (Panama / JNI), C++
 * or Python host flattens a MultiBodySystemReadOnly once into mh_model_desc
 * (recipe: tools/MultiBodySystemFactories.java:401-470,782-868 -- see
 * INTEGRATION.md), then calls mh_rnea / mh_aba / mh_crba with state matrices
 * laid out exactly like the DMatrixRMaj column vectors Mecano uses, stacked
 * along a new leading batch dimension.
 *
 * Conventions (all identical to the reference; B is the only new dimension):
 *   - rigid transform X[12] = { R row-major (9), p (3) } maps coordinates of a
 *     frame into its parent frame: x_parent = R * x_child + p
 *     (ReferenceFrame.getTransformToParent()).
 *   - spatial vectors are ordered angular(3) then linear(3).
 *   - SixDoF configuration = quaternion (x, y, z, s) then position (x, y, z)
 *     (multiBodySystem/interfaces/SixDoFJointReadOnly.java:21-26); it is
 *     normalised on input like Euclid's Quaternion.set does.  SixDoF velocity /
 *     acceleration / effort = (angular, linear) expressed in the frame after
 *     the joint (multiBodySystem/SixDoFJoint.java:64-70).
 *   - gravity is the vector g; the root acceleration is set to -g, expressed in
 *     the root body-fixed frame (InverseDynamicsCalculator.java:343-348).
 *   - external wrenches are per body, expressed in (and about the origin of)
 *     that body's body-fixed (CoM) frame (InverseDynamicsCalculator.java:469-472).
 *   - the mass matrix is dense row-major nv x nv with both triangles filled and
 *     zeros for unrelated branches (CompositeRigidBodyMassMatrixCalculator.java:298,841-845).
 *   - row r of a state matrix belongs to the joint DoF (or configuration entry)
 *     whose entry in dof_indices (cfg_indices) equals r: the
 *     JointMatrixIndexProvider contract
 *     (multiBodySystem/interfaces/JointMatrixIndexProvider.java:71-123).
 *
 * Threading: a model handle is READ-ONLY after mh_model_create and may be shared by any number of host threads and streams.  What
 * compute calls write besides their outputs -- device workspace, scratch matrices, staging buffers, the hand-off flags and the error word
 * of the bias-split forward dynamics -- belongs to a CONTEXT: mh_context_create(model) makes one per host thread / per stream, and a call
 * names it in opts->context.  Calls that leave opts->context NULL use the model's built-in default context and are then subject to the
 * rule of the reference's calculators (one per thread: their scratch fields, InverseDynamicsCalculator.java:706-707): one host thread
 * and one stream at a time per context.  Contexts of one model are independent of each other; so are different models.
 *
 * Calls with device pointers are ASYNCHRONOUS on opts->stream: they return once the work is enqueued.  A failure that shows only while
 * the work runs is therefore reported later: by mh_model_check (synchronises the stream and reports for one context), by
 * mh_stream_synchronize (reports for every context), by the *_host entry points (synchronous: they check before they return) and at the
 * latest by the context's next forward-dynamics call.  One such failure exists: a bias-split forward dynamics launch (small batches of a
 * model with a tree-split code object, mh_aba_f64 / mh_rnea_aba_f64) whose consumer workgroup waited longer than MH_ZV_WAIT_MS
 * (environment, default 2000) for its producer; the accelerations of those 64 configurations are then written as NaN, never as numbers.
 *
 * Last bits: mh_aba_f64 / mh_rnea_aba_f64 choose the formulation of forward dynamics by batch size (bias split while every job gets a CU
 * of its own, one-job tree split up to one group of 64 configurations per CU, beyond that bias and inertia job fused in one workgroup --
 * or two launches where the code object has no fused kernel; MH_ZV / MH_ZVF / MH_ZVB in the environment force each off or on).  The
 * formulations agree to about 1e-13 relative, not bit for bit: the same configuration evaluated inside batches of different sizes -- e.g.
 * in shards of different sizes on different ranks -- may differ in its last bits.  MH_ZV=0 MH_ZVF=0 MH_ZVB=0 pins the one-job form.
 * (Inverse dynamics and the mass matrix have one formulation per code object: their results do not depend on the batch size -- with one
 * exception: beyond one group of 64 configurations per CU mh_rnea_aba_f64 forms its efforts as h + M(q) qdd inside the forward-dynamics
 * launch, within ~1e-15 relative of mh_rnea_f64's, not bit for bit; MH_ZVF_PAIR=0 in the environment keeps the two launches.)
 *
 * No function throws or aborts; every entry point returns an mh_status and
 * mh_last_error() gives a thread-local message.  The library never falls back
 * to a CPU implementation: without a usable HIP device every compute call
 * returns MH_ERR_NO_DEVICE.
 */
#ifndef MECANO_HIP_H
#define MECANO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_ABI_VERSION 5

/* ---- status codes (the Java shim maps them back to Mecano's exception types) ---- */
typedef enum mh_status
{
   MH_OK = 0,
   MH_ERR_INVALID_ARGUMENT = 1,   /* IllegalArgumentException / NullPointerException        */
   MH_ERR_BAD_DIMENSION = 2,      /* MatrixDimensionException (ForwardDynamicsCalculator.java:522-533) */
   MH_ERR_UNSUPPORTED_JOINT = 3,  /* joint kind outside the mh_joint_type enumeration         */
   MH_ERR_LOOP_CLOSURE = 4,       /* kinematic loops: unsupported, as in ForwardDynamicsCalculator.java:207-211 */
   MH_ERR_BAD_TOPOLOGY = 5,       /* parent[] is not a forest / index maps are not a permutation */
   MH_ERR_BAD_AXIS = 6,           /* 1-DoF axis is not a unit vector                          */
   MH_ERR_NO_DEVICE = 7,          /* no HIP device / kernels not loadable                     */
   MH_ERR_HIP = 8,                /* a HIP runtime call failed (message has the HIP error)     */
   MH_ERR_OUT_OF_MEMORY = 9,
   MH_ERR_NOT_RESERVED = 10,      /* batch larger than mh_reserve()d while allocation is forbidden */
   MH_ERR_SINGULAR = 11           /* reserved: the device path does not test joint-space inertias for definiteness -- like the reference's
                                     unguarded 1/D (ForwardDynamicsCalculator.java:1183) a singular block shows as inf / nan in qdd */
} mh_status;

/* ---- joint kinds ---- */
typedef enum mh_joint_type
{
   MH_JOINT_REVOLUTE = 0,  /* multiBodySystem/RevoluteJoint.java   nq=1 nv=1 */
   MH_JOINT_PRISMATIC = 1, /* multiBodySystem/PrismaticJoint.java  nq=1 nv=1 */
   MH_JOINT_SIXDOF = 2,    /* multiBodySystem/SixDoFJoint.java     nq=7 nv=6 */
   MH_JOINT_FIXED = 3,     /* multiBodySystem/FixedJoint.java      nq=0 nv=0 */
   MH_JOINT_PLANAR = 4,    /* multiBodySystem/PlanarJoint.java     nq=3 nv=3   q = (pitch, x, z), qd = (w_y, v_x, v_z) */
   MH_JOINT_SPHERICAL = 5  /* multiBodySystem/SphericalJoint.java  nq=4 nv=3   q = quaternion (x, y, z, s), qd = angular velocity */
} mh_joint_type;

/* ---- memory layout of batched state matrices ---- */
typedef enum mh_layout
{
   MH_LAYOUT_AOS = 0, /* [B][n]: B stacked DMatrixRMaj column vectors (default) */
   MH_LAYOUT_SOA = 1  /* [n][B]: one row per DoF, batch contiguous               */
} mh_layout;

/*
 * Flat description of a MultiBodySystemReadOnly, joints listed in the order of
 * input.getJointMatrixIndexProvider().getIndexedJointsInOrder()
 * (multiBodySystem/interfaces/MultiBodySystemReadOnly.java:57-60,101-104).
 * Joints in getJointsToIgnore() are simply not listed (their subtree inertia,
 * if it must be considered, is lumped by the host into the parent's J/mass/com
 * as InverseDynamicsCalculator.java:832-860 does).
 */
typedef struct mh_model_desc
{
   int32_t n_joints;
   int32_t nq; /* rows of a configuration matrix */
   int32_t nv; /* rows of a velocity / acceleration / effort matrix */
   const int32_t *parent;      /* [n] index of the parent joint (joint.getPredecessor().getParentJoint()), -1 if the predecessor is the root body */
   const int32_t *joint_type;  /* [n] mh_joint_type */
   const double *axis;         /* [3n] joint axis in the joint frame (OneDoFJointReadOnly.getJointAxis()); ignored for SIXDOF/FIXED */
   const double *X_before;     /* [12n] joint.getFrameBeforeJoint().getTransformToParent(); identity when that frame is the parent frame itself (tools/MecanoFactories.java:81-91) */
   const double *X_com;        /* [12n] joint.getSuccessor().getBodyFixedFrame().getTransformToParent() (multiBodySystem/RigidBody.java:170-185) */
   const double *inertia_J;    /* [9n] successor.getInertia().getMomentOfInertia(), row-major, in the body-fixed frame */
   const double *inertia_mass; /* [n]  successor.getInertia().getMass() */
   const double *inertia_com;  /* [3n] successor.getInertia().getCenterOfMassOffset() (normally zero) */
   const int32_t *dof_indices; /* [sum of joint DoFs] getJointDoFIndices(joint), concatenated joint by joint */
   const int32_t *cfg_indices; /* [sum of joint configuration sizes] getJointConfigurationIndices(joint), concatenated */
} mh_model_desc;

/* Per-call switches: mirror of the calculators' setters. */
typedef struct mh_options
{
   int32_t consider_coriolis;      /* InverseDynamicsCalculator.setConsiderCoriolisAndCentrifugalForces (java:291-296); RNEA only; default 1 */
   int32_t consider_accelerations; /* InverseDynamicsCalculator.setConsiderJointAccelerations (java:301-306); RNEA only; default 1 */
   int32_t layout;                 /* mh_layout of every batched matrix of the call */
   int32_t use_root_acceleration;  /* 0 (default): the root body accelerates with (0, -gravity), the `gravity` argument of the call
                                    * (setGravity, InverseDynamicsCalculator.java:318-348, ForwardDynamicsCalculator.java:234-264).
                                    * non-zero: with root_acceleration below; the call's `gravity` argument is ignored and may be NULL */
   void *stream;                   /* hipStream_t to launch on; NULL = the device's null stream */
   double root_acceleration[6];    /* InverseDynamicsCalculator.setRootAcceleration(SpatialAccelerationReadOnly) (java:413-427) and
                                    * ForwardDynamicsCalculator.setRootAcceleration (java:330-343): spatial acceleration of the root body
                                    * (angular x y z, then linear x y z), expressed in the root body's frame, of the root body's frame
                                    * relative to an inertial frame -- what a moving / rotating base contributes; (0, 0, 0, -g) is gravity */
   void *context;                  /* mh_context_t the call's workspace, scratch and flags come from; NULL (default) = the model's own
                                    * default context (then: one host thread and one stream at a time on this model) */
} mh_options;

typedef struct mh_model *mh_model_t;
typedef struct mh_context *mh_context_t;

/* ---- library / device ---- */
int32_t mh_abi_version(void);
/* what a topology-specialised code object (libmecano_hip_topo_<key>.so) must report from its mh_spec_abi() to be accepted by this
 * library build: a hash over the argument structs, record strides and the canonical-frame convention the two share */
uint64_t mh_spec_abi_stamp(void);
/*
 * Build provenance (MH_ABI_VERSION 5).  Every binary carries a hash of what it was compiled from -- FNV-1a 64 over the source files, their
 * headers and the code-generation flags -- as the string "MH_BUILD_ID=<hash>;..." in its file and through these calls:
 *   mh_build_hash()              this library's own sources and flags
 *   mh_spec_sources_hash()       the kernel sources + flags a code object libmecano_hip_topo_<key>.so must have been compiled from to be
 *                                accepted by mh_model_create (it exports the same name; a different hash is refused like a wrong ABI stamp,
 *                                mh_model_kernel_variant says so)
 *   mh_spec_sources_hash_of(dir) the hash of the kernel sources found in `dir` (csrc/), "h" + 16 hex digits + NUL into out[18]: what
 *                                mh_build_code_object checks before it compiles, what mecano_amd/build.py compares instead of file times
 */
const char *mh_build_hash(void);
const char *mh_spec_sources_hash(void);
mh_status mh_spec_sources_hash_of(const char *csrc_dir, char out[18]);
const char *mh_last_error(void);           /* thread-local, never NULL */
mh_status mh_device_count(int32_t *count); /* 0 devices is MH_OK with *count = 0 */
mh_status mh_set_device(int32_t device);   /* device used by subsequent calls of this thread */
void mh_options_default(mh_options *opts); /* coriolis=1, accelerations=1, AoS, null stream */

/* ---- model (replaces the calculators' constructors, InverseDynamicsCalculator.java:226-282) ---- */
mh_status mh_model_create(const mh_model_desc *desc, mh_model_t *model_out);
void mh_model_destroy(mh_model_t model);
int32_t mh_model_nq(mh_model_t model);
int32_t mh_model_nv(mh_model_t model);
int32_t mh_model_n_joints(mh_model_t model);
/* name of the kernel variant compute calls will use for this model: "topo:<key>" when the topology-specialised code object
 * libmecano_hip_topo_<key>.so was found, matches this library build (ABI stamp) and passed the create-time self-check against the
 * run-time-topology kernels; "generic" otherwise, followed by the reason in parentheses when a code object was found but refused */
const char *mh_model_kernel_variant(mh_model_t model);
/*
 * Where this engine consciously departs from the reference (MH_ABI_VERSION 5).  mh_model_create inspects the description and sets:
 *   MH_WARN_NEAR_COORDINATE_AXIS  a revolute axis lies within 1e-7 of +X, +Y or +Z without being that axis.  Mecano then rotates the joint
 *                                 about the EXACT coordinate axis (roll / pitch / yaw closed forms, tools/MecanoFactories.java:51,237-248)
 *                                 while the joint's unit twist keeps the axis as given (multiBodySystem/OneDoFJoint.java:170); the engine
 *                                 uses the given axis for both.  Bound: results differ from Mecano's by <= ~4e-7 relative (instead of 1e-10).
 *                                 Remedy: snap the axis onto the coordinate axis in the description (then both agree to 1e-10).
 *   MH_WARN_TINY_COMPOSITE_MASS   a body's mass plus a child subtree's is under 1e-7: Mecano's SpatialInertia.add skips the
 *                                 renormalisation of the centre of mass (spatial/interfaces/FixedFrameSpatialInertiaBasics.java:174-175);
 *                                 the engine's composite (m, m c, I) stays consistent.  Concerns mh_crba_* / Coriolis / centroidal outputs
 *                                 only (RNEA and ABA never add inertias); bound: <= 1e-6 absolute on H for masses of that size.
 * 0 = the model is in neither class and every output is held to 1e-10 against the reference's arithmetic.  mh_model_warning_text gives
 * the joints concerned ("" when no bit is set; owned by the model); mh_model_create also leaves that text in mh_last_error() while
 * returning MH_OK.
 */
#define MH_WARN_NEAR_COORDINATE_AXIS 1u
#define MH_WARN_TINY_COMPOSITE_MASS 2u
uint32_t mh_model_warnings(mh_model_t model);
const char *mh_model_warning_text(mh_model_t model);

/*
 * Host-only: validates the description and returns the key of its topology (tree shape + joint kinds, in the engine's
 * parents-first order) together with that order's parent / kind arrays.  A topology-specialised code object
 * libmecano_hip_topo_<key>.so placed next to libmecano_hip.so is picked up by mh_model_create (mecano_amd/build.py builds them).
 * key_out holds 16 hex digits + NUL; parents_out / types_out have n_joints entries (either may be NULL).
 */
mh_status mh_topology_key(const mh_model_desc *desc, char key_out[17], int32_t *parents_out, int32_t *types_out);

/*
 * Builds the topology-specialised code object of a model (host-only; runs hipcc -- MH_HIPCC, /opt/rocm/bin/hipcc or the PATH -- on the
 * kernel sources that ship next to the library, csrc/; minutes for a 25-body tree) into out_dir (NULL: next to the library) and returns
 * its path.  Models created afterwards with the same tree shape and joint kinds load it (after the ABI-stamp check and the create-time
 * self-check).  Without it -- and for planar / spherical joints or trees deeper than 16 joints -- a model runs on the run-time-topology
 * kernels (same results; about 2x slower at small batches of a branching tree, 3.5x at device-filling ones).  A host without Python calls
 * this once per robot, e.g. at installation.  With MH_BUILD_FAST=1 in the environment only the tree-split RNEA / ABA / fused kernels for
 * AoS matrices with identity index maps are built -- seconds instead of minutes; every other plan of the model (SoA, per-body outputs,
 * mass matrix, ...) keeps running on the run-time-topology kernels.  MH_AUTO_BUILD=1 (2: the full set) makes mh_model_create do this by
 * itself for a tree it finds no code object for, into MH_SPEC_DIR or next to the library.
 */
mh_status mh_build_code_object(const mh_model_desc *desc, const char *out_dir, char *path_out, size_t path_cap);

/*
 * ---- contexts (see "Threading" at the top) ----
 * A context owns everything a compute call writes besides its outputs; the model handle it was made from stays read-only.  Make one per
 * host thread or stream, pass it in opts->context.  mh_context_reserve is mh_reserve for a context.
 * While contexts of a model exist mh_model_set_joint_source_modes is refused (the contexts hold copies of the joint records' host side).
 * The model is reference-counted by its contexts (they share its device records): mh_model_destroy on a model with live contexts gives
 * up the caller's reference only -- calls through the surviving contexts (with the same handle value) stay valid, no new context can be
 * made -- and the last mh_context_destroy releases the device records.  mh_context_create may run while other threads compute through
 * the model or its contexts.  mh_stream_synchronize reports a pending asynchronous failure of ANY context and clears it -- use
 * mh_model_check where the failing context matters.
 */
mh_status mh_context_create(mh_model_t model, mh_context_t *ctx_out);
void mh_context_destroy(mh_context_t ctx);
mh_status mh_context_reserve(mh_context_t ctx, int64_t max_batch);
/* Synchronises `stream` (NULL = the null stream) and reports failures of the asynchronous calls issued through `ctx` (NULL = the model's
 * default context) that only showed on the device -- see "Calls with device pointers are ASYNCHRONOUS" at the top.  MH_OK: the outputs
 * of every call of this context enqueued on `stream` so far are valid. */
mh_status mh_model_check(mh_model_t model, mh_context_t ctx, void *stream);

/* Pre-allocate device workspace for batches up to max_batch so that compute calls allocate nothing.  After it (and one first call of
 * each entry point, which sets kernel attributes once; a call at any batch size up to max_batch will do) the device-pointer entry points
 * with B <= max_batch only enqueue work on opts->stream -- kernels, memsets, and for a pair call without a fused kernel an event fork /
 * join with a stream of the model's own: they can be captured in a HIP graph and replayed.  The depth-first frame plans of every batch
 * size up to max_batch (both algorithms, both precisions, both layouts, the fp32 fused pair walk) are uploaded here, not at a call
 * (tests/test_gpu_parity.py::test_entry_points_are_graph_capturable,
 * tests/test_gpu_persistent_loops.py::test_reserve_then_capture_every_batch_class).
 * Memory: beside the workspaces, the scratch matrices of the derivative calls and of the AoS form of mh_body_poses_* /
 * mh_geometric_jacobian_* are set aside here for every model and every context, used or not, each while it stays within 4 GiB at
 * max_batch (a larger need is met by the first call that has it).  The kinematics scratch holds the largest target list:
 * max_batch * max(6 * 16 * (nv + 1), 12 * max(16, n_joints) + nv) doubles (the second: the cotangents and the result of
 * mh_body_poses_vjp_*, more than the first only for a model with many fixed joints) -- 23.8 KB per configuration for a 30-DoF model,
 * 97 MB at max_batch = 4096, 3.1 GB at 131 072; from 180 400 configurations on it is left to the first AoS call. */
mh_status mh_reserve(mh_model_t model, int64_t max_batch);

/*
 * ---- compute, DEVICE pointers ----
 * q [B][nq], qd/qdd/tau [B][nv] (or transposed with MH_LAYOUT_SOA), gravity[3] is a HOST pointer,
 * f_ext is NULL or a device pointer [B][n_joints][6] (AoS) / [n_joints*6][B] (SoA) holding, for the
 * successor body of each listed joint, the external wrench (moment, force) in its body-fixed frame.
 * Calls are asynchronous on opts->stream.
 *
 * Aliasing.  "Alias" means the same pointer and the same shape; any other overlap of two arguments is a partial overlap.  The rules hold
 * for the f64 and the f32 form of a call alike; they are checked on the host after the NULL checks, before anything is launched or
 * allocated, and a refused call (MH_ERR_INVALID_ARGUMENT, mh_last_error names the two arguments that overlap) leaves its outputs untouched.
 * mh_rnea_*, mh_aba_*: the output may be exactly one of the call's input state matrices -- qd, the third input (qdd or tau), or q where
 * nq == nv, every joint with degrees of freedom is revolute and its entry of q is its entry of qd (a kernel reads a revolute angle once;
 * prismatic and planar coordinates are read again after the joint's output has been stored).  The aliased call gives the bits of the
 * out-of-place call.  The output never overlaps f_ext; a partial overlap with any input is refused.
 */
mh_status mh_rnea_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd,
                      const double gravity[3], const double *f_ext, const mh_options *opts, double *tau_out);
mh_status mh_aba_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau,
                     const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out);
mh_status mh_crba_f64(mh_model_t model, int64_t B, const double *q, const mh_options *opts, double *H_out);
/*
 * RNEA and ABA of the same B configurations in one call: tau_out = RNEA(q, qd, qdd), qdd_out = ABA(q, qd, tau).  The two are
 * independent.  With a code object the call is ONE launch at every batch size: up to one group of 64 configurations per CU the two run
 * side by side on different workgroups (a 4096-configuration batch is 64 waves, a quarter of what fills an MI355X); beyond that the
 * forward-dynamics kernel also writes tau_out = h + M(q) qdd ("Last bits" above).  Same results as mh_rnea_f64 followed by mh_aba_f64.
 * Because the two run concurrently, tau_out and qdd_out must not overlap q, qd, qdd, tau or each other (MH_ERR_INVALID_ARGUMENT); for
 * in-place use call mh_rnea_f64 and mh_aba_f64 one after the other.
 */
mh_status mh_rnea_aba_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *tau,
                          const double gravity[3], const double *f_ext, const mh_options *opts, double *tau_out, double *qdd_out);

/*
 * InverseDynamicsCalculator.compute + CompositeRigidBodyMassMatrixCalculator.getMassMatrix for the SAME configurations in one call
 * (what a whole-body controller evaluates per tick: algorithms/InverseDynamicsCalculator.java:496-501,
 * algorithms/CompositeRigidBodyMassMatrixCalculator.java:344-348): tau_out [B][nv], H_out [B][nv][nv].  With a code object the two run
 * side by side in ONE launch; otherwise as two launches, concurrently on small batches.  Same arguments as mh_rnea_f64 / mh_crba_f64.
 * Aliasing: tau_out may be qd or qdd.  The mass matrix reads q while the inverse dynamics writes tau_out, so tau_out overlapping q is
 * refused (also where nq == nv), as is H_out overlapping any input or tau_out (MH_ERR_INVALID_ARGUMENT).
 */
mh_status mh_rnea_crba_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                           const double *f_ext, const mh_options *opts, double *tau_out, double *H_out);

/*
 * ---- joint source modes (ForwardDynamicsCalculator.JointSourceMode, ForwardDynamicsCalculator.java:45-57, 400-444) ----
 * modes[n_joints], one per listed joint: MH_EFFORT_SOURCE (tau is the input, qdd the output; the default) or
 * MH_ACCELERATION_SOURCE (the joint is "locked" onto a given acceleration: qdd is the input, tau the output).  NULL resets every
 * joint to MH_EFFORT_SOURCE (resetJointSourceModes, :441-444).  Synchronises the device; not to be called while compute calls
 * on this model are in flight.  While any joint is an acceleration source, forward dynamics goes through mh_aba_locked_f64 and
 * mh_aba_f64 / mh_rnea_aba_f64 return MH_ERR_INVALID_ARGUMENT (they have no acceleration input).
 */
enum
{
   MH_EFFORT_SOURCE = 0,
   MH_ACCELERATION_SOURCE = 1
};
mh_status mh_model_set_joint_source_modes(mh_model_t model, const int32_t *modes);
/* number of joints currently in MH_ACCELERATION_SOURCE mode */
int32_t mh_model_n_acceleration_sources(mh_model_t model);
/*
 * Forward dynamics with acceleration-source joints (ForwardDynamicsCalculator.compute(tau, qdd), :508-520, passes two/three/four
 * :1237-1253, 1284-1297, 1315-1363).  tau [B][nv] is read at the DoFs of the effort-source joints, qdd_in [B][nv] at the DoFs of
 * the acceleration-source joints (it may be NULL when there are none).  qdd_out receives every joint's acceleration (the given
 * ones copied through); tau_out, when not NULL, every joint's effort (the given ones copied through, the efforts that realise the
 * prescribed accelerations computed).  Aliasing: qdd_out is qdd_in or disjoint from every input (q, qd, tau, qdd_in, f_ext); tau_out is
 * tau or disjoint from every input; qdd_out and tau_out are disjoint from each other.  Everything else is refused
 * (MH_ERR_INVALID_ARGUMENT) -- qdd_out == tau among it: the kernel stores a joint's acceleration and then copies its effort through.
 */
mh_status mh_aba_locked_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *qdd_in,
                            const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out, double *tau_out);

/*
 * ---- per-body outputs (RigidBodyAccelerationProvider: InverseDynamicsCalculator.getAccelerationProvider, InverseDynamicsCalculator.java:242-250,
 *      660-663; ForwardDynamicsCalculator.getAccelerationProvider, ForwardDynamicsCalculator.java:170-180, 715-718) ----
 * Same as mh_rnea_f64 / mh_aba_f64, plus for the successor body of every listed joint its spatial acceleration and / or twist relative
 * to the inertial frame, expressed in the body-fixed frame: body_acc_out, body_twist_out [B][n_joints][6] (angular, linear), laid
 * out like f_ext; either may be NULL.  As in the reference the acceleration carries the root acceleration -g, and the RNEA switches
 * apply (consider_coriolis = 0: velocity terms dropped and twists reported as zero).  Models with a tree-split code object, identity
 * index maps and AoS matrices run variants of the tree-split kernels that write them as well; every other case the run-time-topology kernels.
 * Aliasing: tau_out / qdd_out as in mh_rnea_* / mh_aba_*; body_acc_out and body_twist_out must be disjoint from every input, from
 * tau_out / qdd_out and from each other (MH_ERR_INVALID_ARGUMENT otherwise).
 */
mh_status mh_rnea_bodies_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                             const double *f_ext, const mh_options *opts, double *tau_out, double *body_acc_out, double *body_twist_out);
mh_status mh_aba_bodies_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                            const double *f_ext, const mh_options *opts, double *qdd_out, double *body_acc_out, double *body_twist_out);

/*
 * ---- per-joint wrenches (InverseDynamicsCalculator.getComputedJointWrench, InverseDynamicsCalculator.java:578-585, 930-959;
 *      ForwardDynamicsCalculator.getJointWrench, ForwardDynamicsCalculator.java:642-650, 1330-1363) ----
 * Same as mh_rnea_f64 / mh_aba_f64, plus for every listed joint the full 6-D wrench (moment, force) it transmits to its successor body,
 * before projection onto the motion subspace, expressed in the joint's frame after the joint: joint_wrench_out [B][n_joints][6], laid
 * out like f_ext.  tau = S^T wrench.  The forward-dynamics form evaluates, like the reference, a Newton-Euler sweep over the accelerations
 * it has just computed (a second launch on the same stream); it needs every joint to be an effort source.  Run-time-topology kernels.
 * Aliasing: tau_out of mh_rnea_joint_wrenches_f64 as in mh_rnea_*.  qdd_out of mh_aba_joint_wrenches_f64 may be tau and no other input:
 * the second launch reads q, qd and f_ext again, beside the accelerations.  joint_wrench_out must be disjoint from every input and from
 * tau_out / qdd_out.  MH_ERR_INVALID_ARGUMENT otherwise.
 */
mh_status mh_rnea_joint_wrenches_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                                     const double *f_ext, const mh_options *opts, double *tau_out, double *joint_wrench_out);
mh_status mh_aba_joint_wrenches_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                    const double *f_ext, const mh_options *opts, double *qdd_out, double *joint_wrench_out);

/*
 * ---- relative accelerations (RigidBodyAccelerationProvider.getRelativeAcceleration(base, body),
 *      algorithms/interfaces/RigidBodyAccelerationProvider.java:66, 199-235) ----
 * For n_pairs pairs of bodies: the spatial acceleration of body's body-fixed frame with respect to base's, expressed in body's, from the
 * per-body outputs of a previous mh_rnea_bodies_f64 / mh_aba_bodies_f64 call on the same configurations (body_acc, body_twist: DEVICE
 * pointers, [B][n_joints][6]).  base_joints / body_joints are HOST arrays of n_pairs indices into the model's joint list (the successor
 * body of that joint); -1 names the root body, whose acceleration is the root acceleration -g (gravity[3], HOST pointer).
 * opts->consider_coriolis = 0 mirrors a provider that ignores velocities (areVelocitiesConsidered() == false: plain change of frame,
 * body_twist may be NULL).  out [B][n_pairs][6] (MH_LAYOUT_SOA: [n_pairs*6][B]), DEVICE pointer.
 */
mh_status mh_relative_acceleration_f64(mh_model_t model, int64_t B, const double *q, const double *body_acc, const double *body_twist,
                                       const double gravity[3], int32_t n_pairs, const int32_t *base_joints, const int32_t *body_joints,
                                       const mh_options *opts, double *out);

/*
 * ---- joint torque regressor (JointTorqueRegressorCalculator.compute / getJointTorqueRegressorMatrix,
 *      algorithms/JointTorqueRegressorCalculator.java:173-190, 450-453, 749-833; a caller of the inverse dynamics, :118, :181-182, :802-804) ----
 * Y_out [B][nv][10 n_joints], one row-major nv x 10 n matrix per configuration (a DMatrixRMaj each; MH_LAYOUT_SOA: [nv][10 n_joints][B],
 * every store coalesced -- several times faster to produce):  tau = Y pi  for the inverse
 * dynamics without external wrenches, with pi = (mass, com_x, com_y, com_z, Ixx, Ixy, Ixz, Iyy, Iyz, Izz) of every successor body in
 * its body-fixed frame (:877-889; the columns of a body follow SpatialInertiaBasisOption, :514-516).  The ten columns of joint j's
 * successor body start at column 10 j, j in mh_model_desc order -- the reference orders the blocks by the iteration order of a HashMap
 * of rigid bodies (:85, :123, :318-329), which is not specified; getJointTorqueRegressorMatrixBlock(body) (:462-465) is the order-free
 * accessor a shim maps onto this layout.  opts->consider_coriolis / consider_accelerations as in mh_rnea_f64
 * (setConsiderCoriolisAndCentrifugalForces / setConsiderJointAccelerations, :489-502); opts->layout is the layout of q, qd, qdd and Y.
 * first_moment_columns = 0 reproduces the reference: its MCOM_X/Y/Z bases put a centre-of-mass offset on a body of zero mass (:579-581)
 * and every term of the dynamic wrench carries the mass (tools/MecanoTools.java:632-702, 785-822), so those three columns are zero --
 * except with consider_coriolis = 0, where the inverse dynamics passes no twist and computeDynamicMoment leaves c x a unscaled
 * (tools/MecanoTools.java:650-692): the columns then hold the moment e x a, as the reference's do.
 * first_moment_columns = 1 writes d tau / d (m c) there instead (the linear parametrisation used for identification: pi then holds
 * m c in slots 1..3 and the moments of inertia about the origin of the body-fixed frame).  Device pointers, asynchronous on opts->stream;
 * run-time-topology kernel for every model.
 */
mh_status mh_regressor_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                           const mh_options *opts, int32_t first_moment_columns, double *Y_out);
mh_status mh_regressor_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                           const mh_options *opts, int32_t first_moment_columns, float *Y_out);

/*
 * ---- Coriolis matrix (CompositeRigidBodyMassMatrixCalculator.setEnableCoriolisMatrixCalculation(true) + getMassMatrix / getCoriolisMatrix,
 *      algorithms/CompositeRigidBodyMassMatrixCalculator.java:271-274, 344-365, 604-630, 669-768; algorithms/FactorizedBodyInertia.java) ----
 * H_out and C_out [B][nv][nv] row-major (MH_LAYOUT_SOA: [nv*nv][B]):  tau = H qdd + C qd + G.  C is the reference's matrix entry for entry
 * (the factorisation B = v x* I of the body-level Coriolis terms: C qd = RNEA(q, qd, qdd = 0, g = 0), dH/dt = C + C^T); entries of
 * unrelated joints are zero.  Device pointers, asynchronous on opts->stream.  fp64 models with a specialised code object run its
 * compile-time recursion, everything else the run-time-topology kernel.  For big batches MH_LAYOUT_SOA outputs are 3x faster to produce
 * (coalesced stores) than the AoS matrices.
 */
mh_status mh_crba_coriolis_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const mh_options *opts, double *H_out,
                               double *C_out);
mh_status mh_crba_coriolis_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const mh_options *opts, float *H_out, float *C_out);

/*
 * ---- centroidal momentum (CompositeRigidBodyMassMatrixCalculator.getCentroidalMomentumMatrix / getCentroidalConvectiveTermMatrix,
 *      algorithms/CompositeRigidBodyMassMatrixCalculator.java:316-342, 375-420, 801-839) ----
 * A_out [B][6][nv]: h = A qd is the momentum (angular, linear) of the considered bodies in the centroidal momentum frame; b_out [B][6]
 * (may be NULL; needs qd otherwise): dh/dt = A qdd + b.  frame[12] (HOST pointer, R row-major then p; NULL = identity) is the pose of the
 * centroidal momentum frame in the root body frame -- the reference's setCentroidalMomentumFrame(ReferenceFrame) for a frame fixed in the
 * root body; the default NULL is the calculator's default frame (the root body-fixed frame, :190-193).  frame_mode
 * MH_CENTROIDAL_FRAME_AT_COM re-centres that frame on the centre of mass of the considered bodies, i.e. a
 * frames/CenterOfMassReferenceFrame whose parent is `frame`; com_out [B][3] (may be NULL) then receives the centre of mass in `frame`
 * coordinates (algorithms/CenterOfMassCalculator.java:70-91), zeros in MH_CENTROIDAL_FRAME_FIXED mode.
 */
enum
{
   MH_CENTROIDAL_FRAME_FIXED = 0,
   MH_CENTROIDAL_FRAME_AT_COM = 1
};
mh_status mh_centroidal_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double frame[12], int32_t frame_mode,
                            const mh_options *opts, double *A_out, double *b_out, double *com_out);
mh_status mh_centroidal_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const double frame[12], int32_t frame_mode,
                            const mh_options *opts, float *A_out, float *b_out, float *com_out);

/*
 * ---- gravity efforts and their gradient (MultiBodyGravityGradientCalculator.getTauMatrix / getTauGradientMatrix,
 *      algorithms/MultiBodyGravityGradientCalculator.java:397-672) ----
 * tau_out [B][nv]: the joint efforts that hold the system against gravity and the external wrenches -- mh_rnea_* with both switches off,
 * same gravity, same f_ext.  grad_out [B][nv][nv] row-major (MH_LAYOUT_SOA: [nv*nv][B], as H_out of mh_crba_*): entry [i][j] is
 * d tau_i / d q_j, so that tau(q + dq) = tau(q) + grad(q) dq.  dq lives in velocity space: it is the step
 * MultiBodySystemStateIntegrator.integrateFromVelocity applies (for a SixDoF, planar or spherical joint a twist increment in the frame
 * after the joint, not a quaternion delta).  Every external wrench is held constant IN THE WORLD while the configuration varies.
 * Entries of joints neither of which is an ancestor of the other are zero; the kernel writes the whole matrix, zeros included, so
 * grad_out need not be cleared.  The gravity part is symmetric between DoFs of different joints; the external part goes to the
 * [descendant][ancestor] entry only, and with opposite signs to the two entries of a pair of DoFs of one multi-DoF joint.
 * gravity[3] is a HOST pointer, the vector g in the root body frame (not NULL).  f_ext as for mh_rnea_* (may be NULL).  Either output may
 * be NULL, not both (MH_ERR_INVALID_ARGUMENT).  opts->consider_coriolis, opts->consider_accelerations, opts->use_root_acceleration and
 * opts->root_acceleration are ignored: the calculator has no velocities, no accelerations and no moving base.  Ignored subtrees are
 * lumped by the host as for every other call (mh_model_desc).  Device pointers, asynchronous on opts->stream; run-time-topology kernel
 * for every model; after mh_reserve the call allocates nothing.
 */
mh_status mh_gravity_gradient_f64(mh_model_t model, int64_t B, const double *q, const double gravity[3], const double *f_ext,
                                  const mh_options *opts, double *tau_out, double *grad_out);
mh_status mh_gravity_gradient_f32(mh_model_t model, int64_t B, const float *q, const double gravity[3], const float *f_ext,
                                  const mh_options *opts, float *tau_out, float *grad_out);

/*
 * ---- inverse apparent inertia of bodies (MultiBodyResponseCalculator.computeRigidBodyApparentSpatialInertiaInverse /
 *      computeRigidBodyApparentLinearInertiaInverse, applyRigidBodyWrench + getAccelerationChangeProvider,
 *      algorithms/MultiBodyResponseCalculator.java:288-500, 608-627, 859-862, 1191-1338) ----
 * How target body b accelerates when a wrench acts on target body a, for n_targets bodies at once: the 6 x 6 blocks of W = J H^-1 J^T,
 * from the articulated-body recursion itself (neither J nor H is formed), at zero velocity.
 * target_joints (HOST, [n_targets]): positions in the model's joint list; the target is that joint's successor body, as in f_ext and
 * body_acc_out.  Duplicates are allowed (two contact points on one body, with different poses).
 * target_poses (HOST, [n_targets][12], R row-major 9 + p 3, or NULL = identity): the reference's inertiaFrame as a constant pose relative
 * to the target's body-fixed frame (the frame body_acc_out of mh_aba_bodies_* is expressed in).  The wrench (moment, force) acts at and
 * is expressed in that frame; the response is the change of the spatial acceleration (angular, linear) of that frame's origin, expressed
 * in it.  The change of frame is the plain motion / force transform (no velocities, hence no Coriolis terms).  R must be a rotation to 1e-9.
 * blocks = MH_APPARENT_BLOCKS_DIAGONAL: W_out [B][n_targets][6][6] (MH_LAYOUT_SOA: [n_targets * 36][B]), block k = response of target k to a
 * wrench on itself; its lower-right 3 x 3 is the inverse apparent linear inertia.
 * blocks = MH_APPARENT_BLOCKS_COUPLED: W_out [B][6 K][6 K] row-major, K = n_targets (MH_LAYOUT_SOA: [(6 K)^2][B]), block (b, a) = response of
 * target b to a unit wrench on target a.  Its diagonal blocks carry the bits of the DIAGONAL call; W is symmetric up to rounding (every
 * block is computed, none mirrored).
 * The model's joint source modes hold, as in mh_aba_locked_*: an MH_ACCELERATION_SOURCE joint keeps a zero change of acceleration and hands
 * the articulated inertia of its subtree to its parent undiminished.  Every entry of W_out is written (no memset needed), nothing outside
 * it.  W_out must not overlap q.  MH_ERR_INVALID_ARGUMENT: NULL q / W_out / target_joints, n_targets outside 1 ... MH_MAX_APPARENT_TARGETS,
 * a joint index out of range, an unknown blocks value, a pose that is no rotation, W_out overlapping q.  B = 0 returns MH_OK and touches
 * nothing.  Device pointers, asynchronous on opts->stream; run-time-topology kernel for every model; targets and poses travel as kernel
 * arguments: nothing is uploaded, and after mh_reserve the call allocates nothing.
 */
enum { MH_APPARENT_BLOCKS_DIAGONAL = 0, MH_APPARENT_BLOCKS_COUPLED = 1 };
#define MH_MAX_APPARENT_TARGETS 16
mh_status mh_apparent_inertia_inverse_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *target_joints,
                                          const double *target_poses, int32_t blocks, const mh_options *opts, double *W_out);
mh_status mh_apparent_inertia_inverse_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *target_joints,
                                          const double *target_poses, int32_t blocks, const mh_options *opts, float *W_out);

/*
 * ---- body poses and geometric Jacobians (the frame tree's getTransformToDesiredFrame towards the root body frame;
 *      GeometricJacobianCalculator.setKinematicChain / getJacobianMatrix / getConvectiveTerm,
 *      algorithms/GeometricJacobianCalculator.java:148-158, 249-279, 316-377, 578-633; the chain is
 *      MultiBodySystemTools.collectJointPath, tools/MultiBodySystemTools.java:170-207) ----
 * Conventions of both calls, those of mh_apparent_inertia_inverse_* and mh_relative_acceleration_f64:
 * target_joints / base_joints (HOST, [n_targets]): positions in the model's joint list; a position names that joint's successor body, -1
 * names the root body.  Duplicates are allowed.  target_poses (HOST, [n_targets][12], R row-major 9 + p 3, or NULL = identity): a constant
 * pose of the target frame relative to the target's body-fixed frame (for the root body: relative to the root body frame); R must be a
 * rotation to 1e-9.  Targets, bases and poses travel as kernel arguments: nothing is uploaded, and after mh_reserve the calls allocate
 * nothing and can be captured in a graph (AoS outputs of more than 4 GiB at the reserved batch are staged in scratch the first such call
 * allocates).  B = 0 returns MH_OK and touches nothing.  Every entry of every output is written, zeros included, and nothing outside it.
 * Outputs must not overlap inputs or each other.  MH_ERR_INVALID_ARGUMENT: such an overlap, NULL q / output / target_joints, n_targets
 * outside its range, a joint index outside -1 ... n_joints - 1, a pose that is no rotation, conv_out without qd.  Ignored subtrees (they
 * are not in the joint list), the index maps and MH_LAYOUT_SOA are honoured as everywhere else; quaternions are normalised on input.
 * Device pointers, asynchronous on opts->stream, contexts honoured; run-time-topology kernels for every model.
 *
 * mh_body_poses_*: pose_out [B][n_targets][12] (MH_LAYOUT_SOA: [12 n_targets][B]), R row-major then p: the pose of every target frame in
 * the root body frame -- the frame `gravity` is expressed in: x_root = R x + p.  target_joints = NULL with n_targets = n_joints (and
 * target_poses = NULL): the body-fixed frame of every body, in joint order.  Otherwise 1 <= n_targets <= MH_MAX_KINEMATIC_TARGETS.
 *
 * mh_geometric_jacobian_*: J_out [B][6 n_targets][nv] row-major (MH_LAYOUT_SOA: [6 n_targets * nv][B]); block k, rows 6 k ... 6 k + 5
 * (angular, then linear), is the geometric Jacobian of target k:  J qd  is the twist of the target frame relative to the body
 * base_joints[k] (NULL: the root body for every target), expressed in the target frame.  Columns are indexed like tau.  Columns of joints
 * off the chain between base and target are zero; joints on the base's side of the common ancestor enter with their unit twists
 * inverted, as in the reference (:268-271).  With every base at the root the stacked matrix is the J of MH_APPARENT_BLOCKS_COUPLED:
 * W = J H^-1 J^T.  conv_out [B][n_targets][6] (MH_LAYOUT_SOA: [6 n_targets][B]; may be NULL, needs qd otherwise; qd may be NULL when it
 * is): the convective term Jdot qd of getConvectiveTerm (:316-377, 629-633), the acceleration of the target relative to the base at zero
 * joint accelerations in the reference's convention -- what mh_relative_acceleration_f64 returns after an mh_rnea_bodies_f64 call with
 * qdd = 0, re-expressed in the target pose.  The Jacobian frame is always rigidly attached to the end effector (a constant pose in the
 * target body): the only case in which the reference's convective term is valid (its warning, :288, :587, :605).
 */
#define MH_MAX_KINEMATIC_TARGETS 16
mh_status mh_body_poses_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *target_joints,
                            const double *target_poses, const mh_options *opts, double *pose_out);
mh_status mh_body_poses_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *target_joints,
                            const double *target_poses, const mh_options *opts, float *pose_out);
mh_status mh_geometric_jacobian_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets,
                                    const int32_t *base_joints, const int32_t *target_joints, const double *target_poses,
                                    const mh_options *opts, double *J_out, double *conv_out);
mh_status mh_geometric_jacobian_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets,
                                    const int32_t *base_joints, const int32_t *target_joints, const double *target_poses,
                                    const mh_options *opts, float *J_out, float *conv_out);

/*
 * ---- reverse mode of the kinematics: the gradient of a loss on body poses with respect to q, and J^T w without forming J
 *      (GeometricJacobianCalculator.getJointTorques, algorithms/GeometricJacobianCalculator.java:477-484, is J^T w through the matrix) ----
 * target_joints, base_joints, target_poses, layouts, index maps, contexts and quaternion normalisation: the conventions of mh_body_poses_*
 * and mh_geometric_jacobian_* above, word for word.  One outward sweep for the poses and one inward sweep that adds the wrenches up towards
 * the root and reads each joint's share as S^T f: nv numbers per configuration are written, no 6 K x nv matrix.
 *
 * mh_body_poses_vjp_*: g_pose [B][n_targets][12] (MH_LAYOUT_SOA: [12 n_targets][B]) is the cotangent of pose_out of mh_body_poses_* for the
 * same targets and poses, entry for entry (9 for R row-major, then 3 for p); the nine need not be tangent to the rotations.  gq_out [B][nv]
 * (MH_LAYOUT_SOA: [nv][B]), indexed like tau:  gq_out[j] = sum_k sum_e g_pose[k][e] d pose_out[k][e] / d q_j, a step of q being the
 * velocity-space step of mh_configuration_add_* (the chart of every other derivative of the library).  In closed form, with (R_k, p_k) the
 * pose of target k, M = R_k^T G_R, n_k = (M32 - M23, M13 - M31, M21 - M12) and f_k = R_k^T g_p:  gq = sum_k J_k^T (n_k; f_k), J_k the
 * rooted Jacobian of mh_geometric_jacobian_* for that target and pose.  target_joints = NULL with n_targets = n_joints (and target_poses =
 * NULL): the cotangents of the body-fixed frames of every body, in joint order.  The root body as a target contributes nothing.
 *
 * mh_jacobian_transpose_*: wrench [B][n_targets][6] (MH_LAYOUT_SOA: [6 n_targets][B]), moment then force, in the target frame at its
 * origin.  tau_out [B][nv] (MH_LAYOUT_SOA: [nv][B]) = sum_k J_k^T w_k, J_k exactly the block mh_geometric_jacobian_* returns for
 * (base_joints[k], target_joints[k], pose k); base_joints = NULL: every base is the root body.  With a moving base w_k acts on the target
 * body and its opposite on the base body: joints above their common ancestor receive nothing.  target_joints = NULL is refused.
 *
 * Both: every entry of the output is written exactly once -- exact zeros for joints on no chain and for DoF indices no joint owns -- and
 * nothing outside it.  Joint source modes play no part.  Rows are independent: a non-finite q or cotangent spoils its own row only.
 * B = 0 or nv = 0 returns MH_OK and touches nothing.  MH_ERR_INVALID_ARGUMENT: the argument errors of the forward calls, NULL g_pose /
 * wrench / output with B > 0, any overlap of the output with an input.  Device pointers, asynchronous on opts->stream; after mh_reserve /
 * mh_context_reserve the calls allocate nothing and can be captured in a graph.
 */
mh_status mh_body_poses_vjp_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *target_joints,
                                const double *target_poses, const double *g_pose, const mh_options *opts, double *gq_out);
mh_status mh_body_poses_vjp_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *target_joints,
                                const double *target_poses, const float *g_pose, const mh_options *opts, float *gq_out);
mh_status mh_jacobian_transpose_f64(mh_model_t model, int64_t B, const double *q, int32_t n_targets, const int32_t *base_joints,
                                    const int32_t *target_joints, const double *target_poses, const double *wrench,
                                    const mh_options *opts, double *tau_out);
mh_status mh_jacobian_transpose_f32(mh_model_t model, int64_t B, const float *q, int32_t n_targets, const int32_t *base_joints,
                                    const int32_t *target_joints, const double *target_poses, const float *wrench,
                                    const mh_options *opts, float *tau_out);

/*
 * ---- inverse of the joint-space inertia matrix (columns of H^-1: MultiBodyResponseCalculator.applyJointWrench and the recursion behind
 *      it, algorithms/MultiBodyResponseCalculator.java:685-735, 1206-1338; a joint's diagonal block is
 *      computeJointApparentInertiaInverse, :512-590) ----
 * H^-1 of every configuration, or some of its columns, from the articulated-body recursion: H is not formed and nothing dense is
 * factorised.  It is d qdd / d tau of the forward dynamics.
 * columns (HOST) = NULL: all nv columns, n_columns is ignored; Hinv_out [B][nv][nv] row-major (MH_LAYOUT_SOA: [nv * nv][B]), laid out and
 * indexed like H_out of mh_crba_* (the model's DoF index map).
 * columns given: 1 ... MH_MAX_INVERSE_COLUMNS DoF indices in that same index space, duplicates allowed; Hinv_out [B][nv][n_columns]
 * (MH_LAYOUT_SOA: [nv * n_columns][B]), column k = H^-1 e_columns[k].  A listed column carries the bits of that column of the full call.
 * Column c is what mh_aba_* returns for qd = 0, gravity = 0, no external wrenches and tau = e_c.  The model's joint source modes hold as
 * in mh_aba_locked_* with qdd_in = 0: rows and columns of the DoFs of an MH_ACCELERATION_SOURCE joint are zero, the rest is the inverse of
 * H restricted to the DoFs of the effort-source joints.  Rows and columns of DoF indices no joint owns are zero.  H^-1 is symmetric up
 * to rounding (every entry is computed, none mirrored).
 * Every entry of Hinv_out is written (no memset needed), nothing outside it.  Hinv_out must not overlap q.  MH_ERR_INVALID_ARGUMENT: NULL
 * q / Hinv_out, with columns given n_columns outside 1 ... MH_MAX_INVERSE_COLUMNS or an index outside 0 ... nv - 1, Hinv_out overlapping
 * q.  B = 0 returns MH_OK and touches nothing, as does a model with nv = 0.  opts->consider_coriolis, consider_accelerations and the root
 * acceleration play no part.  Device pointers, asynchronous on opts->stream; run-time-topology kernel for every model; the columns travel
 * as kernel arguments: nothing is uploaded, and after mh_reserve the call allocates nothing.
 */
#define MH_MAX_INVERSE_COLUMNS 64
mh_status mh_mass_matrix_inverse_f64(mh_model_t model, int64_t B, const double *q, int32_t n_columns, const int32_t *columns,
                                     const mh_options *opts, double *Hinv_out);
mh_status mh_mass_matrix_inverse_f32(mh_model_t model, int64_t B, const float *q, int32_t n_columns, const int32_t *columns,
                                     const mh_options *opts, float *Hinv_out);

/*
 * ---- first-order derivatives of the inverse and the forward dynamics at a moving state (no calculator of the reference: its
 *      MultiBodyGravityGradientCalculator is the qd = 0, qdd = 0 special case, which mh_rnea_derivatives_* reproduces) ----
 * mh_rnea_derivatives_*: tau_out [B][nv] (may be NULL) = mh_rnea_* of the same inputs; dtau_dq_out and dtau_dqd_out [B][nv][nv] row-major
 * (MH_LAYOUT_SOA: [nv * nv][B], laid out and indexed like grad_out of mh_gravity_gradient_*): entry [i][j] is d tau_i / d q_j, respectively
 * d tau_i / d qd_j.  Either matrix may be NULL, not both (MH_ERR_INVALID_ARGUMENT).  dq is a velocity-space step, exactly as in
 * mh_gravity_gradient_*: the step mh_integrate_* applies (for a SixDoF, planar or spherical joint a twist increment in the frame after the
 * joint); the COMPONENTS of qd and qdd are held fixed while q moves, and every external wrench is held constant IN THE WORLD.
 * opts->consider_coriolis = 0 evaluates at qd = 0 (qd may then be NULL) and writes d tau / d qd as zeros; opts->consider_accelerations = 0
 * evaluates at qdd = 0 (qdd may then be NULL).  opts->use_root_acceleration / root_acceleration are honoured as in mh_rnea_* (gravity may
 * then be NULL).  The model's joint source modes play no part.  Every entry of both matrices is written, zeros of unrelated joints
 * included (no memset needed), nothing outside the outputs.  The outputs must not overlap the inputs or each other
 * (MH_ERR_INVALID_ARGUMENT).  B = 0 or nv = 0 returns MH_OK and touches nothing.  Analytic, O(n depth) per configuration: one launch of a
 * run-time-topology kernel for every model.  Device pointers, asynchronous on opts->stream, contexts honoured; after mh_reserve the call
 * allocates nothing.
 * mh_aba_derivatives_*: with qdd = mh_aba_*(q, qd, tau), dqdd_dq_out = -H^-1 d tau / d q and dqdd_dqd_out = -H^-1 d tau / d qd at that qdd
 * (same layout, same meaning of dq; at least one of the two, MH_ERR_INVALID_ARGUMENT otherwise), and d qdd / d tau = H^-1.  qdd_out [B][nv]
 * and Hinv_out [B][nv][nv] may be NULL: they then go to scratch of the context, which mh_reserve / mh_context_reserve set aside while it
 * stays within 4 GiB (a larger need is met at the first such call).  Launches composed on opts->stream: forward dynamics (whichever plan
 * mh_aba_* takes), the kernel above, the full mh_mass_matrix_inverse_*, and a product kernel that replaces each matrix D by -H^-1 D in
 * place, column by column (H^-1 is read as its transpose: symmetric up to rounding).  nv <= 4096.  A model with MH_ACCELERATION_SOURCE
 * joints is refused (MH_ERR_INVALID_ARGUMENT), as by mh_aba_*.  The outputs must not overlap the inputs or each other.
 */
mh_status mh_rnea_derivatives_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                                  const double *f_ext, const mh_options *opts, double *tau_out, double *dtau_dq_out, double *dtau_dqd_out);
mh_status mh_rnea_derivatives_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                                  const float *f_ext, const mh_options *opts, float *tau_out, float *dtau_dq_out, float *dtau_dqd_out);
mh_status mh_aba_derivatives_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                 const double *f_ext, const mh_options *opts, double *qdd_out, double *dqdd_dq_out, double *dqdd_dqd_out,
                                 double *Hinv_out);
mh_status mh_aba_derivatives_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                                 const float *f_ext, const mh_options *opts, float *qdd_out, float *dqdd_dq_out, float *dqdd_dqd_out,
                                 float *Hinv_out);

/*
 * ---- reverse-mode gradients (vector-Jacobian products) of the inverse and the forward dynamics: what backpropagation through the dynamics
 *      needs, without any of the matrices above (no calculator of the reference) ----
 * mh_rnea_vjp_*: for a cotangent u [B][nv] of the efforts, gq_out[j] = sum_i u_i d tau_i / d q_j, gqd_out[j] = sum_i u_i d tau_i / d qd_j and
 * gqdd_out = H(q) u, each [B][nv] (MH_LAYOUT_SOA: [nv][B]) and each optional -- at least one (MH_ERR_INVALID_ARGUMENT otherwise).  The
 * matrices are exactly those of mh_rnea_derivatives_*: dq is a velocity-space step, the COMPONENTS of qd and qdd are held fixed, every
 * external wrench is held constant IN THE WORLD.  opts->consider_coriolis = 0 evaluates at qd = 0 (qd may then be NULL) and writes gqd_out
 * as zeros; opts->consider_accelerations = 0 evaluates at qdd = 0 (qdd may then be NULL); opts->use_root_acceleration / root_acceleration
 * are honoured (gravity may then be NULL).  u = 0 gives zeros.  Every entry of the outputs given is written once, zeros at DoF indices no
 * joint owns included (no memset needed), nothing outside them.  Analytic, O(n) per configuration, 3 nv numbers written instead of
 * 2 nv^2: ONE launch of a run-time-topology kernel for every model; after mh_reserve the call allocates nothing.
 * mh_aba_vjp_*: for a cotangent w [B][nv] of qdd = mh_aba_*(q, qd, tau): gtau_out = mu = H^-1 w, gq_out = -(d tau / d q)^T mu and
 * gqd_out = -(d tau / d qd)^T mu at that qdd, i.e. w^T d qdd / d (q, qd, tau) with the matrices of mh_aba_derivatives_*; at least one of
 * the three (MH_ERR_INVALID_ARGUMENT otherwise).  qdd_out [B][nv] may be NULL.  Launches composed on opts->stream: forward dynamics
 * (whichever plan mh_aba_* takes), forward dynamics again at rest without root acceleration and wrenches for H^-1 w, the kernel above.
 * No nv x nv matrix is read, written or reserved: the scratch is 2 B nv elements of the context (qdd and mu where the caller takes
 * neither), set aside by mh_reserve / mh_context_reserve, after which the call only enqueues work (graph-capturable).
 * Both: a model with MH_ACCELERATION_SOURCE joints is refused (MH_ERR_INVALID_ARGUMENT).  The outputs must not overlap the inputs (u / w
 * included) or each other.  B = 0 or nv = 0 returns MH_OK and touches nothing.  Device pointers, asynchronous on opts->stream, layouts,
 * index maps and contexts honoured.
 */
mh_status mh_rnea_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                          const double *f_ext, const double *u, const mh_options *opts, double *gq_out, double *gqd_out, double *gqdd_out);
mh_status mh_rnea_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                          const float *f_ext, const float *u, const mh_options *opts, float *gq_out, float *gqd_out, float *gqdd_out);
mh_status mh_aba_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                         const double *f_ext, const double *w, const mh_options *opts, double *qdd_out, double *gq_out, double *gqd_out,
                         double *gtau_out);
mh_status mh_aba_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                         const float *f_ext, const float *w, const mh_options *opts, float *qdd_out, float *gq_out, float *gqd_out,
                         float *gtau_out);

/*
 * ---- the chart of the velocity-space derivatives, and the linearisation of the simulation step ----
 * mh_configuration_add_*: q_out [B][nq] = q (+) dq, dq [B][nv]: the pure configuration step every gradient above is defined in --
 * MultiBodySystemStateIntegrator.integrateFromVelocity with dt = 1 and twist dq (tools/MultiBodySystemStateIntegrator.java:164-243), per
 * joint: 1-DoF q + dq; SixDoF Q' = Q exp(dth), p' = p + R(Q) dp with the INITIAL orientation; spherical the rotational half; planar the same
 * rule in the XZ plane; fixed joints have nothing to update.  (mh_integrate_* with qd = dq is NOT this step: its double integrator adds a
 * w x v term.)  Entries of q_out no joint owns are not written.  q_out may be q itself; any other overlap is refused.
 * mh_configuration_difference_*: the dq_out [B][nv] with q0 (+) dq_out = q1: rotations as the rotation vector of Q0^-1 Q1 in its shortest
 * form (|dth| <= pi; both quaternions are normalised on input), dp = R(Q0)^T (p1 - p0), a planar pitch as the plain difference (not
 * wrapped).  DoF entries no joint owns are written as 0.  dq_out overlaps neither input.
 * Both: device pointers, asynchronous on opts->stream, opts->layout, index maps and contexts honoured; one elementwise
 * run-time-topology kernel, nothing allocated (graph-capturable); B = 0 returns MH_OK and touches nothing.
 * mh_aba_integrate_derivatives_*: the discrete pair (A, B) of the step mh_aba_integrate_f64 takes -- mh_aba_* followed by mh_integrate_*
 * with step dt --, x' = step(x, u), dx' = A dx + B du with x = (q, qd), dx = (dq, dqd) in R^(2 nv) and u = tau.  dq is a velocity-space
 * step in the (+) above and dq' the velocity-space step of q_next, q_next(x (+) dx) (-) q_next(x); dqd and dqd' are plain component
 * increments (for a SixDoF joint qd_next is expressed in the NEW frame after the joint, as mh_integrate_* returns it); external wrenches
 * are held fixed IN THE WORLD, as in mh_aba_derivatives_*.  A_out [B][2 nv][2 nv] row-major, rows and columns over dq in the model's DoF
 * index space, then dqd; B_out [B][2 nv][nv]; MH_LAYOUT_SOA: [(2 nv)^2][B] and [2 nv nv][B].  Either matrix may be NULL, not both;
 * qdd_out may be NULL; q_next and qd_next may be NULL only together, and given they are what mh_integrate_* gives for the call's qdd (one
 * more launch of the integrator kernel).  Rows and columns of DoF indices no joint owns are zero; every entry of both matrices is
 * written (no memset needed), nothing outside the outputs.  The outputs overlap neither the inputs nor each other -- q_next == q and
 * qd_next == qd included: the matrices are formed from the old state.  dt may be 0 (A = identity on owned DoFs, B = 0, exactly) or
 * negative; a dt that is not finite is MH_ERR_INVALID_ARGUMENT, as are MH_ACCELERATION_SOURCE joints in the model.  B = 0 or nv = 0
 * returns MH_OK and touches nothing.  opts->use_root_acceleration is honoured.  Launches composed on opts->stream: mh_aba_derivatives_*
 * with d qdd / d q, d qdd / d qd and H^-1 in scratch of the context (set aside by mh_reserve / mh_context_reserve while all of it stays
 * within 4 GiB; a larger need is met at the first call), and one assembly kernel that reads each element of the three once and writes
 * each element of A and B once, rows contiguous across lanes in both layouts.  After reserve and one first call the entry point only
 * enqueues work.
 */
mh_status mh_configuration_add_f64(mh_model_t model, int64_t B, const double *q, const double *dq, const mh_options *opts, double *q_out);
mh_status mh_configuration_add_f32(mh_model_t model, int64_t B, const float *q, const float *dq, const mh_options *opts, float *q_out);
mh_status mh_configuration_difference_f64(mh_model_t model, int64_t B, const double *q0, const double *q1, const mh_options *opts,
                                          double *dq_out);
mh_status mh_configuration_difference_f32(mh_model_t model, int64_t B, const float *q0, const float *q1, const mh_options *opts,
                                          float *dq_out);
mh_status mh_aba_integrate_derivatives_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                                           const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out,
                                           double *q_next, double *qd_next, double *A_out, double *B_out);
mh_status mh_aba_integrate_derivatives_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *tau,
                                           const double gravity[3], const float *f_ext, const mh_options *opts, float *qdd_out,
                                           float *q_next, float *qd_next, float *A_out, float *B_out);

/*
 * ---- reverse-mode gradients of the integrator and of the simulation step: what backpropagation through a rollout needs, without the
 *      matrices A and B above (no calculator of the reference) ----
 * mh_integrate_vjp_*: for cotangents gq_next, gqd_next [B][nv] of (dq', dqd') of mh_integrate_*(q, qd, qdd) with step dt, the gradients
 * gq_out, gqd_out, gqdd_out [B][nv] with respect to (dq, dqd, dqdd): the transpose of the integrator's per-joint tangent map, in the
 * conventions of mh_aba_integrate_derivatives_* -- dq and dq' are velocity-space steps of (+), dqd and dqd' component increments, qd_next
 * of a SixDoF joint in the NEW frame.  Neither q nor the joints' poses appear.  The cotangent of the integrator's optional re-expressed
 * qdd_out is not an input: it is taken as zero.  ONE launch of an elementwise run-time-topology kernel, no workspace; joint source modes
 * play no part.
 * mh_aba_integrate_vjp_*: the same for the step mh_aba_* followed by mh_integrate_*: gq_out = A^T g', gqd_out likewise and
 * gtau_out = B^T g' with g' = (gq_next, gqd_next) and the (A, B) of mh_aba_integrate_derivatives_*, external wrenches held IN THE WORLD.
 * qdd_out [B][nv] may be NULL.  Launches composed on opts->stream: forward dynamics (whichever plan mh_aba_* takes), the kernel of
 * mh_integrate_vjp_* (the integrator's own share of gq and gqd, and w = the cotangent of qdd), forward dynamics at rest for H^-1 w, and the
 * adjoint sweep of mh_aba_vjp_*, which adds its share to gq_out and gqd_out -- one launch more than mh_aba_vjp_*; the sweep is dropped where
 * gq_out and gqd_out are both NULL.  No nv x nv matrix is read, written or reserved: the scratch is at most 3 B nv elements of the context
 * (qdd, w and H^-1 w where the caller takes neither qdd_out nor gtau_out), set aside by mh_reserve / mh_context_reserve.  A model with
 * MH_ACCELERATION_SOURCE joints is refused (MH_ERR_INVALID_ARGUMENT), as is gravity == NULL without a root acceleration.
 * Both: every cotangent and gradient is [B][nv] (MH_LAYOUT_SOA: [nv][B]).  Either cotangent may be NULL and is then taken as zero; both
 * NULL is refused.  At least one gradient output must be given (MH_ERR_INVALID_ARGUMENT otherwise).  Every entry of an output given is
 * written once, zeros at DoF indices no joint owns included (cotangent entries there are not read), nothing outside the outputs.  The
 * outputs overlap neither the inputs nor each other.  dt may be 0 (gq_out = gq_next, gqd_out = gqd_next, gqdd_out / gtau_out = 0, exactly)
 * or negative; a dt that is not finite is MH_ERR_INVALID_ARGUMENT.  B = 0 or nv = 0 returns MH_OK and touches nothing.  Device pointers,
 * asynchronous on opts->stream, layouts, index maps and contexts honoured; after mh_reserve / mh_context_reserve the calls only enqueue
 * work (graph-capturable).
 */
mh_status mh_integrate_vjp_f64(mh_model_t model, int64_t B, double dt, const double *qd, const double *qdd, const double *gq_next,
                               const double *gqd_next, const mh_options *opts, double *gq_out, double *gqd_out, double *gqdd_out);
mh_status mh_integrate_vjp_f32(mh_model_t model, int64_t B, double dt, const float *qd, const float *qdd, const float *gq_next,
                               const float *gqd_next, const mh_options *opts, float *gq_out, float *gqd_out, float *gqdd_out);
mh_status mh_aba_integrate_vjp_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                                   const double gravity[3], const double *f_ext, const double *gq_next, const double *gqd_next,
                                   const mh_options *opts, double *qdd_out, double *gq_out, double *gqd_out, double *gtau_out);
mh_status mh_aba_integrate_vjp_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *tau,
                                   const double gravity[3], const float *f_ext, const float *gq_next, const float *gqd_next,
                                   const mh_options *opts, float *qdd_out, float *gq_out, float *gqd_out, float *gtau_out);

/*
 * ---- forward-mode derivatives (JVP) of the dynamics, the integrator and the simulation step: the matrices of mh_rnea_derivatives_*,
 *      mh_aba_derivatives_* and mh_aba_integrate_derivatives_* times DIRECTIONS, without forming them (no calculator of the reference) ----
 * The conventions are those of the matrices: dq is a velocity-space step of mh_configuration_add_*, the components of qd, qdd and tau
 * move by plain increments, external wrenches are held IN THE WORLD, dq_next is the velocity-space step of q_next and qd_next of a SixDoF
 * joint is in the NEW frame.  Every direction and every tangent output is [B][nv] (MH_LAYOUT_SOA: [nv][B]), with the strides and index
 * maps of qd.
 * mh_rnea_jvp_*: dtau_out = (d tau / d q) dq + (d tau / d qd) dqd + H dqdd at (q, qd, qdd).  ONE launch of a run-time-topology kernel, the
 * tangent of the Newton-Euler recursion: two sweeps, O(n), nv numbers written per configuration.  consider_coriolis,
 * consider_accelerations and use_root_acceleration are honoured as by mh_rnea_vjp_*: with consider_coriolis = 0 qd and dqd may be NULL and
 * dqd contributes nothing, with consider_accelerations = 0 qdd may be NULL (H dqdd is formed all the same).
 * mh_aba_jvp_*: dqdd_out = H^-1 (dtau - (d tau / d q) dq - (d tau / d qd) dqd) at qdd = mh_aba_*(q, qd, tau), which goes to qdd_out
 * (may be NULL).  Launches composed on opts->stream: forward dynamics (whichever plan mh_aba_* takes, with the caller's switches), the
 * tangent sweep at (q, qd, qdd) with both switches on, which writes the right-hand side, and forward dynamics at rest on it.  Without dq
 * and dqd the sweep is dropped and the first launch runs only for qdd_out; dqdd_out then has the bits of mh_aba_vjp_*'s gtau_out for
 * w = dtau.  Scratch: at most 2 B nv elements of the context (qdd where the caller takes none, and the right-hand side).
 * mh_integrate_jvp_*: (dq_next_out, dqd_next_out) = the integrator's per-joint tangent map at (qd, qdd) and step dt applied to
 * (dq, dqd, dqdd); mh_integrate_vjp_* is its transpose.  ONE elementwise launch, no workspace; joint source modes play no part.  At least
 * one of the two outputs must be given.
 * mh_aba_integrate_jvp_*: (dq_next_out, dqd_next_out) = A (dq, dqd) + B dtau with the (A, B) of mh_aba_integrate_derivatives_*, and
 * dqdd_out as mh_aba_jvp_* gives it: exactly mh_aba_jvp_* followed by mh_integrate_jvp_*, four launches, at most 3 B nv elements of
 * scratch.  At least one of dqdd_out, dq_next_out and dqd_next_out must be given; qdd_out may be NULL.
 * All: a direction that is NULL is zero and is not read; all directions NULL is MH_ERR_INVALID_ARGUMENT.  All-zero directions give exact
 * zeros.  Every entry of an output given is written once, zeros at DoF indices no joint owns included (direction entries there are not
 * read), nothing outside the outputs.  The outputs overlap neither the inputs, directions included, nor each other.  dt may be 0
 * (dq_next = dq, dqd_next = dqd exactly on owned DoFs) or negative; a dt that is not finite is MH_ERR_INVALID_ARGUMENT, as are
 * MH_ACCELERATION_SOURCE joints in the model and gravity == NULL without a root acceleration (mh_integrate_jvp_* takes neither).  B = 0 or
 * nv = 0 returns MH_OK and touches nothing.  Device pointers, asynchronous on opts->stream, layouts, index maps and contexts honoured; the
 * scratch is what mh_reserve / mh_context_reserve set aside for the reverse-mode calls, after which the calls only enqueue work
 * (graph-capturable).
 */
mh_status mh_rnea_jvp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double gravity[3],
                          const double *f_ext, const double *dq, const double *dqd, const double *dqdd, const mh_options *opts,
                          double *dtau_out);
mh_status mh_rnea_jvp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                          const float *f_ext, const float *dq, const float *dqd, const float *dqdd, const mh_options *opts,
                          float *dtau_out);
mh_status mh_aba_jvp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                         const double *f_ext, const double *dq, const double *dqd, const double *dtau, const mh_options *opts,
                         double *qdd_out, double *dqdd_out);
mh_status mh_aba_jvp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                         const float *f_ext, const float *dq, const float *dqd, const float *dtau, const mh_options *opts,
                         float *qdd_out, float *dqdd_out);
mh_status mh_integrate_jvp_f64(mh_model_t model, int64_t B, double dt, const double *qd, const double *qdd, const double *dq,
                               const double *dqd, const double *dqdd, const mh_options *opts, double *dq_next_out, double *dqd_next_out);
mh_status mh_integrate_jvp_f32(mh_model_t model, int64_t B, double dt, const float *qd, const float *qdd, const float *dq,
                               const float *dqd, const float *dqdd, const mh_options *opts, float *dq_next_out, float *dqd_next_out);
mh_status mh_aba_integrate_jvp_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                                   const double gravity[3], const double *f_ext, const double *dq, const double *dqd, const double *dtau,
                                   const mh_options *opts, double *qdd_out, double *dqdd_out, double *dq_next_out, double *dqd_next_out);
mh_status mh_aba_integrate_jvp_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *tau,
                                   const double gravity[3], const float *f_ext, const float *dq, const float *dqd, const float *dtau,
                                   const mh_options *opts, float *qdd_out, float *dqdd_out, float *dq_next_out, float *dqd_next_out);

/*
 * ---- inverse and forward dynamics with per-configuration inertial parameters: B different robots of one topology and geometry
 *      (domain randomisation, identification by simulation error, payload sweeps; no calculator of the reference evaluates a batch) ----
 * pi (DEVICE) is [B][n_joints][10], MH_LAYOUT_SOA: [10 n_joints][B] (opts->layout, as for every other matrix of the call).  The ten
 * numbers of joint j's successor body, j in mh_model_desc order, are (mass, com_x, com_y, com_z, Jxx, Jxy, Jxz, Jyy, Jyz, Jzz):
 * inertia_mass, inertia_com and the symmetric part of inertia_J with their mh_model_desc meaning (J about the origin of the body-fixed
 * frame, in its axes) -- the parameter order of mh_regressor_*.  Fixed joints have a block too (their successor carries inertia); a body
 * that had an ignored subtree lumped into it by the host is parametrised by its lumped values.  The call replaces what the description
 * gave for inertia and nothing else: topology, joint frames, axes and index maps stay the model's.
 * mh_model_inertial_parameters: the model's own values in this layout, pi_out (HOST) [n_joints][10]; the matching call with them in
 * every row reproduces mh_rnea_* / mh_aba_* (to rounding: the device applies the host's map from the ten numbers to its inertia record).
 * Gravity, f_ext, opts->root_acceleration, the two switches of mh_rnea_*, stream and context behave as in mh_rnea_* / mh_aba_*; while any
 * joint is MH_ACCELERATION_SOURCE, mh_aba_parameters_* returns MH_ERR_INVALID_ARGUMENT as mh_aba_* does.  pi = NULL is
 * MH_ERR_INVALID_ARGUMENT.  A pi that is no physical inertia is not diagnosed: like the reference's unguarded 1/D it shows as inf / nan
 * in that row only, and the call returns MH_OK.  Aliasing as in mh_rnea_* / mh_aba_*: the output may be qd, the third input, or q under
 * the conditions given there; it never overlaps f_ext or pi, and a partial overlap is refused.  Run-time-topology kernels for
 * every model (mh_params_kernels.h); device pointers, asynchronous on opts->stream; after mh_reserve and one first call the entry points
 * only enqueue work (graph-capturable).
 */
mh_status mh_model_inertial_parameters(mh_model_t model, double *pi_out);
mh_status mh_rnea_parameters_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *pi,
                                 const double gravity[3], const double *f_ext, const mh_options *opts, double *tau_out);
mh_status mh_rnea_parameters_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *pi,
                                 const double gravity[3], const float *f_ext, const mh_options *opts, float *tau_out);
mh_status mh_aba_parameters_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *pi,
                                const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out);
mh_status mh_aba_parameters_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *pi,
                                const double gravity[3], const float *f_ext, const mh_options *opts, float *qdd_out);

/*
 * ---- reverse-mode gradients of the two calls above with respect to the inertial parameters: what a descent on pi needs (identification
 *      by simulation error, fitting a payload, a learned residual inertia), without the regressor (no calculator of the reference) ----
 * mh_rnea_parameters_vjp_*: for a cotangent u [B][nv] of the efforts of mh_rnea_parameters_*(q, qd, qdd, pi),
 * gpi_out[r][j][k] = sum_i u_i d tau_i / d pi[r][j][k], laid out like pi ([B][n_joints][10], MH_LAYOUT_SOA: [10 n_joints][B]), with respect
 * to the ten numbers themselves (mass, com, J) -- not to (m, m c, J): the call applies the chain rule with the row's pi, the only use it
 * makes of pi.  opts->consider_coriolis = 0 evaluates at qd = 0 (qd may then be NULL), opts->consider_accelerations = 0 at qdd = 0 (qdd
 * may then be NULL); opts->use_root_acceleration / root_acceleration are honoured (gravity may then be NULL).  External wrenches do not
 * enter: tau is affine in them.  u = 0 gives zeros, and the block of a body outside the subtrees of the joints where u is not zero is
 * zero.  Every entry of gpi_out is written once (no memset needed), fixed joints' blocks included, nothing outside it.  Analytic, O(n) per
 * configuration, one outward sweep and no inward one, 10 n_joints numbers written where mh_regressor_* writes nv 10 n_joints: ONE launch
 * of a run-time-topology kernel for every model (mh_params_vjp_kernels.h) in the model's own workspace plan.  Joint source modes play
 * no part.
 * mh_aba_parameters_vjp_*: for a cotangent w [B][nv] of qdd = mh_aba_parameters_*(q, qd, tau, pi): gtau_out = mu = H(pi)^-1 w and
 * gpi_out = w^T d qdd / d pi = -mu^T d tau / d pi at that qdd (the kernel above with u = mu, negated).  qdd_out and gtau_out [B][nv] may be
 * NULL.  Launches composed on opts->stream: mh_aba_parameters_* for qdd, again at rest without root acceleration and wrenches with
 * tau = w for mu, the kernel above.  The scratch is 2 B nv elements of the context (qdd and mu where the caller takes neither), set
 * aside by mh_reserve / mh_context_reserve.  A model with MH_ACCELERATION_SOURCE joints is refused (MH_ERR_INVALID_ARGUMENT).
 * Both: pi, u / w or gpi_out = NULL is MH_ERR_INVALID_ARGUMENT, as is an output that overlaps an input (u / w and pi included) or another
 * output.  B = 0 returns MH_OK and touches nothing.  A pi row that is no physical inertia or not finite is not diagnosed: it shows as
 * inf / nan in that row's outputs only.  The state gradients of mh_rnea_vjp_* / mh_aba_vjp_* at per-configuration parameters are those
 * of mh_rnea_parameters_state_vjp_* / mh_aba_parameters_state_vjp_* below.  Device pointers, asynchronous on opts->stream, layouts, index
 * maps and contexts honoured; after mh_reserve / mh_context_reserve the calls only enqueue work (graph-capturable).
 */
mh_status mh_rnea_parameters_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *pi,
                                     const double gravity[3], const double *u, const mh_options *opts, double *gpi_out);
mh_status mh_rnea_parameters_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *pi,
                                     const double gravity[3], const float *u, const mh_options *opts, float *gpi_out);
mh_status mh_aba_parameters_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *pi,
                                    const double gravity[3], const double *f_ext, const double *w, const mh_options *opts, double *qdd_out,
                                    double *gtau_out, double *gpi_out);
mh_status mh_aba_parameters_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *pi,
                                    const double gravity[3], const float *f_ext, const float *w, const mh_options *opts, float *qdd_out,
                                    float *gtau_out, float *gpi_out);

/*
 * ---- reverse-mode gradients of the same two calls with respect to the state AND the inertial parameters in one call: what
 *      backpropagation through a rollout of a robot whose parameters are being learned needs (fitting pi from measured trajectories, a
 *      policy over randomised robots, a payload and a controller optimised together; no calculator of the reference) ----
 * The contract is the union of mh_rnea_vjp_* / mh_aba_vjp_* and mh_rnea_parameters_vjp_* / mh_aba_parameters_vjp_*.
 * mh_rnea_parameters_state_vjp_*: for a cotangent u [B][nv] of the efforts of mh_rnea_parameters_*(q, qd, qdd, pi): gq_out = u^T d tau / d q,
 * gqd_out = u^T d tau / d qd, gqdd_out = H(pi) u, each [B][nv] (MH_LAYOUT_SOA: [nv][B]), and gpi_out[r][j][k] = sum_i u_i d tau_i / d pi[r][j][k],
 * laid out like pi ([B][n_joints][10], MH_LAYOUT_SOA: [10 n_joints][B]) and taken with respect to the ten numbers themselves.  The matrices
 * contracted are those of mh_rnea_derivatives_*, evaluated with the inertias of row r -- the velocity-space chart, the components of qd and
 * qdd fixed, external wrenches held IN THE WORLD --, none of them formed.  opts->consider_coriolis = 0 evaluates at qd = 0 (qd may then be
 * NULL; gqd_out is exact zeros), opts->consider_accelerations = 0 at qdd = 0 (qdd may then be NULL); opts->use_root_acceleration is
 * honoured (gravity may then be NULL).  u = 0 gives exact zeros in every output.  ONE launch of a run-time-topology kernel for every model
 * (mh_params_state_vjp_kernels.h): the two sweeps of mh_rnea_vjp_* in that call's workspace plan, with every body's inertia read from the
 * row's pi in both, and the ten derivatives of a body formed in the outward one -- where mh_rnea_vjp_* beside mh_rnea_parameters_vjp_*
 * runs two outward sweeps and one inward.  No scratch.
 * mh_aba_parameters_state_vjp_*: for a cotangent w [B][nv] of qdd = mh_aba_parameters_*(q, qd, tau, pi): gtau_out = mu = H(pi)^-1 w,
 * gq_out = -mu^T d tau / d q, gqd_out = -mu^T d tau / d qd and gpi_out = -mu^T d tau / d pi at that qdd (the kernel above with u = mu, negated),
 * which are w^T d qdd / d q, w^T d qdd / d qd, w^T d qdd / d tau and w^T d qdd / d pi with the matrices of mh_aba_derivatives_* at H(pi_r).
 * qdd_out [B][nv] may be NULL; it is written as mh_aba_parameters_* writes it (entries at DoF indices no joint owns are left alone).
 * Launches composed on opts->stream: mh_aba_parameters_* for qdd, again at rest without root acceleration and wrenches with tau = w for mu
 * (behind one memset), the kernel above -- three launches where mh_aba_vjp_* beside mh_aba_parameters_vjp_*
 * takes six; the sweep is dropped where only gtau_out is asked for.  The scratch is 2 B nv elements of the context (qdd and mu where the
 * caller takes neither), set aside by mh_reserve / mh_context_reserve.
 * Both: each gradient output may be NULL and is then neither formed nor written; at least one of gq_out, gqd_out, gqdd_out / gtau_out and
 * gpi_out must be given (MH_ERR_INVALID_ARGUMENT otherwise).  Every entry of an output given is written once (no memset needed), zeros at
 * DoF indices no joint owns and the blocks of fixed joints included, nothing outside the outputs.  pi == NULL is
 * MH_ERR_INVALID_ARGUMENT, as are MH_ACCELERATION_SOURCE joints in the model, gravity == NULL without a root acceleration, and an output
 * that overlaps an input (u / w and pi included) or another output.  B = 0 or nv = 0 returns MH_OK and touches nothing.  A pi row that is
 * no physical inertia or not finite is not diagnosed: it shows as inf / nan in that row's outputs only.  Device pointers, asynchronous on
 * opts->stream, layouts, index maps and contexts honoured; after mh_reserve / mh_context_reserve the calls only enqueue work
 * (graph-capturable).
 */
mh_status mh_rnea_parameters_state_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *pi,
                                           const double gravity[3], const double *f_ext, const double *u, const mh_options *opts, double *gq_out,
                                           double *gqd_out, double *gqdd_out, double *gpi_out);
mh_status mh_rnea_parameters_state_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *pi,
                                           const double gravity[3], const float *f_ext, const float *u, const mh_options *opts, float *gq_out,
                                           float *gqd_out, float *gqdd_out, float *gpi_out);
mh_status mh_aba_parameters_state_vjp_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double *pi,
                                          const double gravity[3], const double *f_ext, const double *w, const mh_options *opts, double *qdd_out,
                                          double *gq_out, double *gqd_out, double *gtau_out, double *gpi_out);
mh_status mh_aba_parameters_state_vjp_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *pi,
                                          const double gravity[3], const float *f_ext, const float *w, const mh_options *opts, float *qdd_out,
                                          float *gq_out, float *gqd_out, float *gtau_out, float *gpi_out);

/*
 * ---- forward dynamics under bilateral constraints on body frames, and the velocity-level twin for touch-down (the consumer of the
 *      apparent inertias: MultiBodyResponseCalculator's applyRigidBodyWrench / propagateImpulse are the pieces, the reference has no
 *      calculator that solves for the wrench; algorithms/MultiBodyResponseCalculator.java:39-41, 608-627, 640, 836) ----
 * "How does the robot accelerate while these frames are held", "what is its velocity after these frames are stopped": the equality-
 * constrained solve underneath every contact method.  Inequalities and friction cones of point contacts: mh_contact_impulse_* below;
 * other inequalities and complementarity conditions stay with the caller.
 * Targets: n_targets K = 1 ... MH_MAX_CONSTRAINT_TARGETS; target_joints (HOST, [K]) and target_poses (HOST, [K][12] or NULL = identity)
 * exactly as in mh_apparent_inertia_inverse_*: a position names that joint's successor body, duplicates are allowed, the pose is
 * relative to the body-fixed frame, R must be a rotation to 1e-9, the root body is no target.
 * Rows: target_rows (HOST, [K]) is a 6-bit mask per target, bit i constrains row i of the target frame (rows 0-2 angular, 3-5 linear):
 * 0b111000 is a point contact, 0b111111 a weld.  At least one bit must be set over all targets; m = the number of bits set <= 48.
 * active (DEVICE int32, [B][K]; MH_LAYOUT_SOA: [K][B]; NULL = every row active): a mask of the same form per configuration.  A row takes
 * part in configuration r only where its bit is set in both masks; bits outside target_rows[k] are ignored.
 * The constrained motion is that of the target frame relative to the root body, expressed in the target frame, as
 * mh_geometric_jacobian_* defines it with every base at the root: J qdd + Jdot qd (its conv_out), respectively J qd.  Gravity and the
 * root acceleration enter through the dynamics only.
 * compliance eps (>= 0) is added to the diagonal of the constraint-space matrix.  With eps = 0 a rank-deficient set of rows is the
 * caller's error: a configuration whose factorisation meets a pivot that is not positive and finite gets quiet NaN in all its outputs;
 * no other configuration is affected and no error is raised.
 *
 * mh_aba_constrained_*: with J_c the active selected rows of J and c those of Jdot qd,
 *    H qdd + h(q, qd, g, f_ext) = tau + J_c^T lambda,     J_c qdd + c + eps lambda = a_des
 * a_des (DEVICE) [B][K][6] (MH_LAYOUT_SOA: [6 K][B]; NULL = zeros; entries of rows that are not constrained are not read).  qdd_out
 * [B][nv].  lambda_out [B][K][6] (same layout; may be NULL): the wrench (moment, force) the constraint applies to target k's body, acting
 * at and expressed in the target frame; unconstrained and inactive rows hold exactly 0.0.  Equivalently qdd_out = mh_aba_*(q, qd, tau,
 * g, f_ext + sum_k X_k^T lambda_k) with X_k the body-to-target motion transform of pose k.  opts->use_root_acceleration is honoured as in
 * mh_aba_* (gravity may then be NULL).
 * mh_constraint_impulse_*: qd_out = qd + H^-1 J_c^T Lambda with J_c qd_out + eps Lambda = v_des (same shape as a_des; NULL = zeros: the
 * frames stop; restitution is the caller's choice of v_des).  impulse_out as lambda_out.  The change of velocity is the forward dynamics
 * at rest, without gravity, with Lambda as the only wrench.  Entries of qd_out no joint owns hold those of qd.
 *
 * Both: launches composed on opts->stream -- forward dynamics with per-body accelerations (impulse: the inverse dynamics' outward sweep
 * for the twists), mh_apparent_inertia_inverse_* (COUPLED) into scratch, one constraint kernel (L D L^T in place, one lane per
 * configuration), forward dynamics again (whichever plan mh_aba_* takes).  Scratch of the context: B * ((6 K)^2 + 6 K + 12 n_joints + nv)
 * elements; mh_reserve / mh_context_reserve set it aside for K = MH_MAX_CONSTRAINT_TARGETS in fp64 while that stays within 4 GiB (a
 * larger need is met by the first call) -- 21.5 KB per configuration for the 30-DoF humanoid, 88 MB at max_batch = 4096.  After reserve
 * and one first call the entry points only enqueue work (graph-capturable).  The outputs overlap neither the inputs (active and a_des /
 * v_des among them: the second launch reads the state again) nor each other.  MH_ERR_INVALID_ARGUMENT: such an overlap; NULL q / qd /
 * tau / qdd_out / target_joints / target_rows; K out of range; a joint index outside 0 ... n_joints - 1; a mask with bits >= 6, or no bit
 * set at all; a negative or NaN compliance; a pose that is no rotation; MH_ACCELERATION_SOURCE joints in the model (as by mh_aba_*).
 * B = 0 returns MH_OK and touches nothing.  Index maps, MH_LAYOUT_SOA and contexts are honoured as everywhere else.
 */
#define MH_MAX_CONSTRAINT_TARGETS 8
mh_status mh_aba_constrained_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                 const double *f_ext, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                                 const int32_t *target_rows, const int32_t *active, const double *a_des, double compliance, const mh_options *opts,
                                 double *qdd_out, double *lambda_out);
mh_status mh_aba_constrained_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                                 const float *f_ext, int32_t n_targets, const int32_t *target_joints, const double *target_poses,
                                 const int32_t *target_rows, const int32_t *active, const float *a_des, double compliance, const mh_options *opts,
                                 float *qdd_out, float *lambda_out);
mh_status mh_constraint_impulse_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets, const int32_t *target_joints,
                                    const double *target_poses, const int32_t *target_rows, const int32_t *active, const double *v_des,
                                    double compliance, const mh_options *opts, double *qd_out, double *impulse_out);
mh_status mh_constraint_impulse_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets, const int32_t *target_joints,
                                    const double *target_poses, const int32_t *target_rows, const int32_t *active, const float *v_des,
                                    double compliance, const mh_options *opts, float *qd_out, float *impulse_out);

/*
 * ---- the same between two moving bodies: a hand on the other hand, a tool in a hand, the closing joint of a four-bar or of a parallel
 *      linkage (the reference's forward dynamics skips loop-closure joints) ----
 * Arguments as mh_aba_constrained_* / mh_constraint_impulse_* with base_joints (HOST, [K]) behind target_joints: a position in the joint
 * list names that joint's successor body, -1 the root body; NULL = the root for every target.  The constrained motion is that of target
 * frame k relative to the body of base_joints[k], expressed in the target frame, exactly as mh_geometric_jacobian_* defines it for that
 * base: J qdd + Jdot qd (its conv_out), respectively J qd.  The equations are those above with this J_c and c.
 * lambda_out[k] / impulse_out[k] is the wrench on the TARGET body, at and in the target frame; the base body receives the opposite wrench
 * at the same point: qdd_out = mh_aba_*(q, qd, tau, g, f_ext + sum_k (X_k^T lambda_k on the target body - Z_k^T lambda_k on the base
 * body)) with X_k the constant body-to-target motion transform of pose k and Z_k the motion transform from the base's body-fixed frame
 * to the target frame at q.  Nothing is applied for a root base.
 * Row masks, active, a_des / v_des, compliance, the NaN rule of a bad pivot, exact zeros in rows that take no part, layouts, index maps,
 * contexts and the aliasing rule are those of the rooted calls.  With base_joints NULL or all -1 the call is the rooted one, bit for bit.
 * Composition: as above, with per-body twists beside the accelerations, the apparent inertia inverse for n_app = K + (non-root bases)
 * frames -- the K target frames, then the body-fixed frame of every non-root base, at most 16 -- and a second instantiation of the
 * constraint kernel that forms the relative right-hand side, reduces W to that of the relative motions in place and adds the base's
 * wrench.  Scratch of the context: B * ((6 n_app)^2 + 6 K + 18 n_joints + nv + 12 K) elements, the 12 K for the poses of the target
 * frames in their bases.  mh_reserve / mh_context_reserve keep the size of the rooted calls: a larger need is met by the first call at
 * that batch; after one such call the entry points only enqueue work (graph-capturable).
 * MH_ERR_INVALID_ARGUMENT: everything the rooted calls refuse; a base outside -1 ... n_joints - 1; base_joints[k] == target_joints[k]
 * (the Jacobian would be zero).  B = 0 returns MH_OK and touches nothing.
 */
mh_status mh_aba_constrained_between_f64(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau, const double gravity[3],
                                         const double *f_ext, int32_t n_targets, const int32_t *target_joints, const int32_t *base_joints,
                                         const double *target_poses, const int32_t *target_rows, const int32_t *active, const double *a_des,
                                         double compliance, const mh_options *opts, double *qdd_out, double *lambda_out);
mh_status mh_aba_constrained_between_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                                         const float *f_ext, int32_t n_targets, const int32_t *target_joints, const int32_t *base_joints,
                                         const double *target_poses, const int32_t *target_rows, const int32_t *active, const float *a_des,
                                         double compliance, const mh_options *opts, float *qdd_out, float *lambda_out);
mh_status mh_constraint_impulse_between_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets,
                                            const int32_t *target_joints, const int32_t *base_joints, const double *target_poses,
                                            const int32_t *target_rows, const int32_t *active, const double *v_des, double compliance,
                                            const mh_options *opts, double *qd_out, double *impulse_out);
mh_status mh_constraint_impulse_between_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets,
                                            const int32_t *target_joints, const int32_t *base_joints, const double *target_poses,
                                            const int32_t *target_rows, const int32_t *active, const float *v_des, double compliance,
                                            const mh_options *opts, float *qd_out, float *impulse_out);

/*
 * ---- frictional point contacts: the inequality-constrained twin of mh_constraint_impulse_* -- a foot that can lift off, press or slide ----
 * K = 1 ... MH_MAX_CONTACT_TARGETS contact points; target_joints and target_poses (HOST) exactly as in mh_constraint_impulse_*.  The
 * contact point is the origin of the target frame.  Per configuration, with
 *    u_k      linear velocity of target frame k relative to the root body, in the target frame (rows 3-5 of J qd of
 *             mh_geometric_jacobian_* with every base at the root),
 *    lambda_k the impulse on the target body at that point, in the target frame,
 *    n_k      the unit contact normal: given per configuration in the ROOT BODY frame, pointing from the obstacle into the robot,
 *             normalised on input and brought into the target frame, n_k = R_pose^T R_body(q)^T n^_k,
 *    mu_k >= 0 the friction coefficient, v_k the least normal velocity after the impulse (Baumgarte and restitution terms are the
 *             caller's choice of v_k), eps >= 0 the compliance,
 * the call returns the unique minimiser of the cone-constrained convex problem (Anitescu's time-stepping relaxation, the model MuJoCo uses)
 *    minimise 1/2 lambda^T (S + eps I) lambda + lambda^T b   subject to   n_k.lambda_k >= 0,  |lambda_k - (n_k.lambda_k) n_k| <= mu_k n_k.lambda_k
 *    b_k = u_k(qd) - v_k n_k,        qd_out = qd + H^-1 J_c^T lambda,
 * S the symmetrised 3 K x 3 K linear part of W = J H^-1 J^T (mh_apparent_inertia_inverse_*, COUPLED): block (k, l) with l < k as computed,
 * its transpose for (l, k), the lower triangle of a diagonal block mirrored.  At mu = 0 this is the exact frictionless complementarity
 * solution 0 <= n.lambda  _|_  n.u+ - v + eps n.lambda >= 0.  A contact whose stick solution lies inside its cone sticks exactly.  A sliding
 * contact has |lambda_t| = mu lambda_n, opposed to its tangential velocity; the relaxation's known artefact is that a sliding contact
 * also lifts off along the normal, at mu times its sliding speed.
 * The iteration: lambda^0 = the linear rows of impulse_init (NULL = zeros), each projected onto its cone (a stale warm start is safe);
 * then n_iterations projected block Gauss-Seidel sweeps, k = 0 ... K - 1 in list order with the newest lambda, closed contacts only,
 *    u = b_k + sum_l S_kl lambda_l + eps lambda_k,    rho_k = 1 / (trace S_kk + eps),    lambda_k = Pi_k(lambda_k - rho_k u)
 * (rho_k <= 1 / lambda_max: each block step descends the objective).  Pi_k(x) is the Euclidean projection onto the cone: with s = n.x,
 * t = x - s n, r = |t|: x if r <= mu s; 0 if mu r <= -s; otherwise s' n + (mu s' / r) t with s' = (s + mu r) / (1 + mu^2) -- nonexpansive,
 * with no discontinuous branch.  Where mu > 1 the three cases are evaluated with a = 1 / mu (a r <= s; r <= -a s; s' = a (a s + r) / (1 + a^2),
 * mu s' / r = (a s + r) / ((1 + a^2) r)): no finite mu overflows, and a very large mu is stick -- the projection onto the half space
 * n.x >= 0.  The caller chooses n_iterations (1 ... MH_MAX_CONTACT_ITERATIONS) and reads residual_out.
 * mu (HOST, [K]).  normals (DEVICE) [B][K][3] (MH_LAYOUT_SOA: [3 K][B]; NULL = (0, 0, 1)).  active (DEVICE int32) [B][K] (SoA [K][B];
 * nonzero = contact k is closed in this configuration; NULL = all): an open contact keeps lambda = 0 exactly.  v_normal (DEVICE) [B][K]
 * (SoA [K][B]; NULL = zeros).  impulse_init (DEVICE): the shape of impulse_out; it may be impulse_out itself (in-place warm start).
 * qd_out [B][nv]: qd plus the forward dynamics at rest, without gravity, with sum_k X_k^T impulse_k as the only wrenches; entries no joint
 * owns hold those of qd.  impulse_out [B][K][6] (SoA [6 K][B]; may be NULL): the wrench on the target body at and in the target frame;
 * rows 0-2 and every row of an open contact hold exactly 0.0.  residual_out [B] (may be NULL): the largest |change of an impulse
 * component| in the last sweep.
 * A configuration gets quiet NaN in all of its outputs when trace S_kk + eps of a closed contact is not positive and finite, when the
 * norm of the n^ of a closed contact is not positive and finite, or when b_k of a closed contact or an impulse after the last sweep is
 * not finite (a NaN in qd, in v_normal or in impulse_init: residual_out never reads as converged beside an impulse that is no number);
 * no other configuration changes and no error is raised.
 * Launches composed on opts->stream as for mh_constraint_impulse_*, with the contact solve (one lane per configuration, S in LDS while
 * it fits, otherwise streamed from scratch: the same bits either way) in the place of the factorisation.  Scratch of the context:
 * B * ((6 K)^2 + 6 K + 12 n_joints + nv) elements, which mh_reserve / mh_context_reserve cover; after reserve and one first call the entry
 * point only enqueues work (graph-capturable).  MH_ERR_INVALID_ARGUMENT, outputs untouched: NULL q / qd / qd_out / target_joints / mu;
 * K outside 1 ... MH_MAX_CONTACT_TARGETS; a joint outside 0 ... n_joints - 1; a pose that is no rotation; a mu that is negative, not
 * finite, or beyond the largest finite number of the call's precision (mh_contact_impulse_f32: above 3.4e38); a negative or NaN compliance; n_iterations outside 1 ... MH_MAX_CONTACT_ITERATIONS; MH_ACCELERATION_SOURCE joints in the model;
 * any overlap of an output with an input or another output, except impulse_out == impulse_init exactly.  B = 0 returns MH_OK and
 * touches nothing.  Index maps, MH_LAYOUT_SOA and contexts are honoured as everywhere else.
 */
#define MH_MAX_CONTACT_TARGETS 8
#define MH_MAX_CONTACT_ITERATIONS 4096
mh_status mh_contact_impulse_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets, const int32_t *target_joints,
                                 const double *target_poses, const double *mu, const double *normals, const int32_t *active, const double *v_normal,
                                 const double *impulse_init, double compliance, int32_t n_iterations, const mh_options *opts, double *qd_out,
                                 double *impulse_out, double *residual_out);
mh_status mh_contact_impulse_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets, const int32_t *target_joints,
                                 const double *target_poses, const double *mu, const float *normals, const int32_t *active, const float *v_normal,
                                 const float *impulse_init, double compliance, int32_t n_iterations, const mh_options *opts, float *qd_out,
                                 float *impulse_out, float *residual_out);

/*
 * ---- the same between two moving bodies: a hand on the other hand, a foot on the other leg, fingers on an object that is itself a
 *      floating body of the tree, a link against its neighbour ----
 * Arguments as mh_contact_impulse_* with base_joints (HOST, [K]) behind target_joints, as in the other _between_ calls: a position in the
 * joint list names that joint's successor body, -1 the root body; NULL = the root for every contact.  Per configuration, with
 *    u_k      rows 3-5 of J qd of mh_geometric_jacobian_* for target k with base base_joints[k]: the linear velocity of the contact point
 *             on the target body relative to the base body, in the target frame,
 *    S        the symmetrised linear 3 x 3 blocks of W_rel = J_rel H^-1 J_rel^T, J_rel,k = J_t - Z_k J_b, read exactly as above: block (k, l)
 *             with l < k as computed, its transpose for (l, k), the lower triangle of a diagonal block mirrored,
 *    n_k      still given per configuration in the ROOT BODY frame, pointing from the base body (the obstacle) into the target body, and
 *             brought into the target frame by the target body's pose, n_k = R_pose^T R_body(q)^T n^_k,
 *    lambda_k the impulse on the target body at the origin of the target frame, in the target frame; the base body receives -lambda_k at
 *             the same point: -Z_k^T (0, lambda_k), Z_k the motion transform from the base's body-fixed frame to the target frame at q, as
 *             in mh_constraint_impulse_between_*.  Nothing is applied for a root base,
 * the call returns the minimiser of the same problem with b_k = u_k(qd) - v_k n_k and
 *    qd_out = qd + H^-1 J_rel^T lambda:
 * forward dynamics at rest, without gravity, with sum_k (X_k^T impulse_k on the target body - Z_k^T impulse_k on the base body) as the only
 * wrenches.  Two bodies of the tree exchange momentum and the total is conserved, which no rooted contact can do.
 * The objective, the cone projection (the mu > 1 form through 1 / mu included), the sweep order, rho_k = 1 / (trace S_kk + eps), the warm
 * start, active, v_normal, residual_out and the exact zeros in angular rows and open contacts are those of mh_contact_impulse_*.  The NaN
 * rule is that call's; a configuration whose q makes a pose of either climb non-finite is NaN in all three outputs through b_k.
 * A target and a base may be any two different bodies: ancestor and descendant, two limbs, or a body that is the target of one contact
 * and the base of another; duplicated bases are allowed.  With base_joints NULL or all -1 the call takes the rooted launches and returns
 * the bits of mh_contact_impulse_*.
 * Composition: as mh_contact_impulse_*, with the apparent inertia inverse for n_app = K + (non-root bases) frames -- the K target frames,
 * then the body-fixed frame of every non-root base, one per contact, at most 16 -- and a second set of instantiations of the contact
 * kernel that forms Z_k and the relative b_k, reduces W to W_rel in place over the target blocks (the step of the constraint kernel)
 * before its sweeps, and loads the base.  S in LDS while it fits (9 K (K + 1) / 2 entries per lane whatever the bases are), otherwise
 * streamed from the reduced W: the same bits either way.  Scratch of the context: B * ((6 n_app)^2 + 6 K + 12 n_joints + nv + 12 K)
 * elements, the 12 K for the poses of the target frames in their bases.  mh_reserve / mh_context_reserve keep the size of the rooted call:
 * a larger need is met by the first call at that batch; after one such call the entry point only enqueues work (graph-capturable).
 * MH_ERR_INVALID_ARGUMENT, outputs untouched: everything mh_contact_impulse_* refuses; a base outside -1 ... n_joints - 1;
 * base_joints[k] == target_joints[k] (the Jacobian would be zero).  B = 0 returns MH_OK and touches nothing.  Layouts, index maps,
 * contexts, the stream and the aliasing rule (impulse_out == impulse_init exactly is the one permitted overlap) are those of the rooted call.
 */
mh_status mh_contact_impulse_between_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_targets,
                                         const int32_t *target_joints, const int32_t *base_joints, const double *target_poses, const double *mu,
                                         const double *normals, const int32_t *active, const double *v_normal, const double *impulse_init,
                                         double compliance, int32_t n_iterations, const mh_options *opts, double *qd_out, double *impulse_out,
                                         double *residual_out);
mh_status mh_contact_impulse_between_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_targets,
                                         const int32_t *target_joints, const int32_t *base_joints, const double *target_poses, const double *mu,
                                         const float *normals, const int32_t *active, const float *v_normal, const float *impulse_init,
                                         double compliance, int32_t n_iterations, const mh_options *opts, float *qd_out, float *impulse_out,
                                         float *residual_out);

/*
 * ---- joint limits: a knee that does not fold through itself.  The unilateral twin of the contact call in joint space ----
 * L = n_limits rows, 1 ... MH_MAX_LIMIT_JOINTS.  limit_joints (HOST, [L]): positions in the model's joint list, as target_joints
 * elsewhere; each listed joint must be revolute or prismatic and may be listed once only; the host resolves each to its DoF index d_i
 * and configuration index c_i through the model's index maps.  lower, upper (HOST, [L]) may be -inf / +inf, lower <= upper; they, margin
 * and erp are converted to the call's precision once.  Per configuration and per row i, in the call's precision:
 *    gap_lo = q[c_i] - lower_i,  gap_hi = upper_i - q[c_i];
 *    s_i = +1 if gap_lo <= gap_hi, else -1 (the nearer limit decides the side, the lower limit wins a tie);  gap_i = min(gap_lo, gap_hi);
 *    row i is CLOSED where gap_i <= margin (margin >= 0, finite); every other row is open and keeps impulse 0.0 exactly;
 *    b_i = s_i qd[d_i] + erp gap_i (erp >= 0, finite, in 1/s): a violated limit (gap < 0) is asked to recover at erp |gap|, a row inside
 *          the margin may still approach at erp gap; with erp = 1 / dt this is exactly "do not cross in the next step";
 *    S_ij = s_i s_j (H^-1)[d_i][d_j], read so that S is exactly symmetric: for j < i the entry in row d_i of column j as
 *          mh_mass_matrix_inverse_* computed it, for j > i S_ji, the diagonal from column i.
 * The call returns the iterate of
 *    minimise 1/2 lambda^T (S + eps I) lambda + lambda^T b   subject to  lambda >= 0   (closed rows),
 * the linear complementarity problem 0 <= lambda_i  _|_  s_i qd+[d_i] + eps lambda_i + erp gap_i >= 0: frictionless, so exact, with no
 * relaxation artefact.  Start: lambda^0_i = max(0, s_i impulse_init_i) on closed rows (NULL = zeros), 0 on open rows: a stale warm start
 * is safe.  Then n_iterations sweeps (1 ... MH_MAX_LIMIT_ITERATIONS), i = 0 ... L - 1 in list order with the newest lambda, closed rows only:
 *    u = b_i + sum_j S_ij lambda_j + eps lambda_i,    lambda_i = max(0, lambda_i - rho_i u),    rho_i = 1 / (S_ii + eps).
 * qd_out [B][nv] = qd + sum over the CLOSED rows, in list order, of (s_i lambda_i) (column d_i of H^-1); entries no joint owns hold those
 * of qd; a configuration with no closed row returns the bits of qd.  impulse_out [B][L] (SoA [L][B]; may be NULL) = s_i lambda_i, the
 * generalised impulse on joint i, positive pushing q up; open rows hold exactly 0.0; it may be impulse_init itself (in-place warm start),
 * the only permitted overlap.  residual_out [B] (may be NULL): the largest |change of a lambda_i| in the last sweep.
 * A configuration gets quiet NaN in all three outputs when q[c_i] of a listed joint is NaN (or infinite), when S_ii + eps of a closed row
 * is not positive and finite, when b_i or impulse_init_i of a closed row is not finite, or when a lambda after the last sweep is not
 * finite; no other configuration changes and no error is raised.
 * Two launches on opts->stream: the listed columns of H^-1 (the kernel of mh_mass_matrix_inverse_*) into the context's scratch as
 * [nv L][B], then the solve (one lane per configuration; S in LDS while (L (L + 1) / 2 + 3 L) 64 elements fit 160 KB -- L <= 22 in fp64,
 * L <= 32 in fp32 -- otherwise streamed from the columns: the same bits either way), which also forms qd_out from those columns: no
 * second forward-dynamics launch.  Scratch of the context: B * nv * L elements; mh_reserve / mh_context_reserve keep their size: a
 * larger need is met by the first call at that batch; after reserve and one first call the entry point only enqueues work
 * (graph-capturable).  Workspace: that of mh_mass_matrix_inverse_* with L columns, which mh_reserve covers.
 * MH_ERR_INVALID_ARGUMENT, outputs untouched, checked before anything is launched: NULL model / q / qd / qd_out / limit_joints / lower /
 * upper; L outside 1 ... MH_MAX_LIMIT_JOINTS; a joint outside 0 ... n_joints - 1, not revolute or prismatic, or listed twice;
 * lower > upper or a NaN limit; margin, erp or compliance negative, NaN or infinite (compliance 0 is allowed); n_iterations outside
 * 1 ... MH_MAX_LIMIT_ITERATIONS; MH_ACCELERATION_SOURCE joints in the model; any overlap of an output with an input or with another
 * output other than impulse_out == impulse_init exactly.  B = 0 returns MH_OK and touches nothing.  Layouts, index maps, the stream and
 * contexts are honoured as everywhere else.
 * Beside contacts: the call solves the limits alone; the caller alternates it with mh_contact_impulse_*, each on the free velocity plus
 * the other's change of velocity (block Gauss-Seidel on the joint dual problem, both blocks warm-started; examples/joint_limits_humanoid.py).
 */
#define MH_MAX_LIMIT_JOINTS 64 /* = MH_MAX_INVERSE_COLUMNS */
#define MH_MAX_LIMIT_ITERATIONS 4096
mh_status mh_joint_limit_impulse_f64(mh_model_t model, int64_t B, const double *q, const double *qd, int32_t n_limits, const int32_t *limit_joints,
                                     const double *lower, const double *upper, double margin, double erp, const double *impulse_init,
                                     double compliance, int32_t n_iterations, const mh_options *opts, double *qd_out, double *impulse_out,
                                     double *residual_out);
mh_status mh_joint_limit_impulse_f32(mh_model_t model, int64_t B, const float *q, const float *qd, int32_t n_limits, const int32_t *limit_joints,
                                     const double *lower, const double *upper, double margin, double erp, const float *impulse_init,
                                     double compliance, int32_t n_iterations, const mh_options *opts, float *qd_out, float *impulse_out,
                                     float *residual_out);

/*
 * ---- state integration (MultiBodySystemStateIntegrator.doubleIntegrateFromAcceleration, tools/MultiBodySystemStateIntegrator.java:365-441,
 *      503-575, 710-733): the step downstream of forward dynamics, so that a simulation loop never leaves the device ----
 * One explicit constant-acceleration step of size dt for every joint of every configuration: 1-DoF q' = q + dt qd + dt^2/2 qdd,
 * qd' = qd + dt qdd; 6-DoF joints integrate the pose with the rotation vector dt w + dt^2/2 dw appended to the quaternion and
 * re-express twist and acceleration in the new frame after the joint, exactly as the reference does.  q_out [B][nq], qd_out [B][nv]
 * and (optional, may be NULL) qdd_out [B][nv] may be their own inputs (in-place step: q_out == q, qd_out == qd, qdd_out == qdd); any other
 * overlap of an output with an input or with another output is refused (MH_ERR_INVALID_ARGUMENT).  Entries no considered joint owns are
 * not written.
 * Device pointers, asynchronous on opts->stream; opts->layout as for the other calls.
 */
mh_status mh_integrate_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *qdd,
                           const mh_options *opts, double *q_out, double *qd_out, double *qdd_out);
/*
 * One simulation step on the device: qdd_out = ABA(q, qd, tau) followed by one integrator step of size dt, q_next / qd_next =
 * integrate(q, qd, qdd_out).  Same results as mh_aba_f64 followed by mh_integrate_f64 (ForwardDynamicsCalculator.compute +
 * MultiBodySystemStateIntegrator.doubleIntegrateFromAcceleration; the loop of MultiBodySystemStateIntegratorTest.java:245-250).  Models
 * with a tree-split code object, identity index maps and AoS matrices run it as ONE launch (the new state is formed from the rows the
 * forward-dynamics kernel already holds in LDS); every other case issues the two launches.  Aliasing: q_next may be q and qd_next may be
 * qd; qdd_out must be disjoint from every input and from q_next and qd_next (the step reads it again); any other overlap is refused
 * (MH_ERR_INVALID_ARGUMENT).  qdd_out is the forward-dynamics result (not re-expressed by the step).
 */
mh_status mh_aba_integrate_f64(mh_model_t model, int64_t B, double dt, const double *q, const double *qd, const double *tau,
                               const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out, double *q_next,
                               double *qd_next);
mh_status mh_integrate_f32(mh_model_t model, int64_t B, double dt, const float *q, const float *qd, const float *qdd,
                           const mh_options *opts, float *q_out, float *qd_out, float *qdd_out);

mh_status mh_rnea_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd,
                      const double gravity[3], const float *f_ext, const mh_options *opts, float *tau_out);
mh_status mh_aba_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau,
                     const double gravity[3], const float *f_ext, const mh_options *opts, float *qdd_out);
mh_status mh_crba_f32(mh_model_t model, int64_t B, const float *q, const mh_options *opts, float *H_out);
/* mh_rnea_aba_f64 in fp32 (BASELINE.json configs[4] evaluates both per step): big batches of wide matrices go through ONE depth-first
 * walk that carries the inverse dynamics through the forward dynamics' first pass (AoS callers: through shared transposed scratch
 * copies of q and qd); otherwise mh_rnea_f32 followed by mh_aba_f32.  The results of those two, to fp32 rounding in the fused walk.
 * The outputs must not overlap the inputs or each other (as for mh_rnea_aba_f64). */
mh_status mh_rnea_aba_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const float *tau,
                          const double gravity[3], const float *f_ext, const mh_options *opts, float *tau_out, float *qdd_out);
/* fp32 forms of the per-body outputs and of forward dynamics with acceleration-source joints (run-time-topology kernels) */
mh_status mh_rnea_bodies_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                             const float *f_ext, const mh_options *opts, float *tau_out, float *body_acc_out, float *body_twist_out);
mh_status mh_aba_bodies_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                            const float *f_ext, const mh_options *opts, float *qdd_out, float *body_acc_out, float *body_twist_out);
mh_status mh_aba_locked_f32(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const float *qdd_in,
                            const double gravity[3], const float *f_ext, const mh_options *opts, float *qdd_out, float *tau_out);

/*
 * ---- compute, HOST pointers (what a JNI / Panama shim with heap or off-heap arrays calls) ----
 * Same arguments, all pointers in host memory; the call copies in, launches, copies out and
 * synchronises before returning.
 */
mh_status mh_rnea_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd,
                           const double gravity[3], const double *f_ext, const mh_options *opts, double *tau_out);
mh_status mh_aba_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double *tau,
                          const double gravity[3], const double *f_ext, const mh_options *opts, double *qdd_out);
mh_status mh_crba_f64_host(mh_model_t model, int64_t B, const double *q, const mh_options *opts, double *H_out);
mh_status mh_rnea_f32_host(mh_model_t model, int64_t B, const float *q, const float *qd, const float *qdd, const double gravity[3],
                           const float *f_ext, const mh_options *opts, float *tau_out);
mh_status mh_aba_f32_host(mh_model_t model, int64_t B, const float *q, const float *qd, const float *tau, const double gravity[3],
                          const float *f_ext, const mh_options *opts, float *qdd_out);
mh_status mh_crba_f32_host(mh_model_t model, int64_t B, const float *q, const mh_options *opts, float *H_out);
/* tau_out = RNEA(q, qd, qdd) and qdd_out = ABA(q, qd, tau) of the same configurations (mh_rnea_aba_f64 per chunk) */
mh_status mh_rnea_aba_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double *qdd, const double *tau,
                               const double gravity[3], const double *f_ext, const mh_options *opts, double *tau_out, double *qdd_out);
/*
 * AoS batches above 1024 configurations travel in chunks through three streams (copy-in, kernels, copy-out overlap).  The copies
 * reach PCIe rate only from / to PINNED host memory: let the host keep its state matrices in memory from mh_host_alloc (Panama: wrap the
 * returned address as a MemorySegment; JNI: NewDirectByteBuffer), or pin existing off-heap buffers once with mh_host_register.
 * Pageable pointers work too, at the runtime's staged-copy rate.
 */
mh_status mh_host_alloc(size_t bytes, void **ptr_out); /* hipHostMalloc */
mh_status mh_host_free(void *ptr);
mh_status mh_host_register(void *ptr, size_t bytes);   /* hipHostRegister: pins a range the host already owns */
mh_status mh_host_unregister(void *ptr);

mh_status mh_crba_coriolis_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const mh_options *opts, double *H_out,
                                    double *C_out);
mh_status mh_centroidal_f64_host(mh_model_t model, int64_t B, const double *q, const double *qd, const double frame[12], int32_t frame_mode,
                                 const mh_options *opts, double *A_out, double *b_out, double *com_out);

/*
 * ---- device memory for hosts without a HIP binding of their own ----
 * A Java shim keeps its state matrices on the device with these and calls the DEVICE-pointer entry points: a simulation loop
 * (mh_aba_integrate_f64 per step) then never crosses PCIe.  Copies are asynchronous on `stream` (NULL = the null stream); pageable
 * host memory is staged by the runtime, pinned memory (mh_host_alloc) is read / written in place -- keep it alive until
 * mh_stream_synchronize returns.
 */
mh_status mh_device_alloc(size_t bytes, void **ptr_out);
mh_status mh_device_free(void *ptr);
mh_status mh_copy_to_device(void *dst_device, const void *src_host, size_t bytes, void *stream);
mh_status mh_copy_to_host(void *dst_host, const void *src_device, size_t bytes, void *stream);
mh_status mh_stream_synchronize(void *stream);

/*
 * ---- multi-GPU: one process per GPU, the batch sharded by rows, RCCL over xGMI ----
 * The reference is single-threaded Java (InverseDynamicsCalculatorTest.java:124-158 times one calculator on one thread) and has no
 * counterpart.  Every configuration is independent and the model is read-only, so the compute entry points above need no collective:
 * each rank calls them on its own rows.  What a host without torch.distributed needs around that (mecano_amd/distributed.py is the
 * same for the Python host) is
 *   mh_shard_range          which rows of a batch a rank owns (contiguous; sizes differ by at most one);
 *   mh_comm_broadcast_host  the robot description (the arrays of mh_model_desc, packed by the host) from the rank that has it;
 *   mh_comm_all_gather_rows the ranks' output rows side by side on every rank, once, after the steps.
 * Rank 0 calls mh_comm_unique_id and carries the MH_COMM_ID_BYTES bytes to the other processes by its own means (a file, a socket, the
 * launcher's environment); every process then calls mh_comm_create on the device it computes on.  librccl.so.1 is opened at the first
 * of these calls (MH_RCCL_LIBRARY overrides the name): MH_ERR_NO_DEVICE when it cannot be.  A communicator is used by one thread at a time.
 */
#define MH_COMM_ID_BYTES 128
typedef struct mh_comm *mh_comm_t;
mh_status mh_shard_range(int64_t B, int32_t rank, int32_t world, int64_t *lo_out, int64_t *hi_out);
mh_status mh_comm_unique_id(void *id_out); /* MH_COMM_ID_BYTES bytes */
mh_status mh_comm_create(const void *id, int32_t rank, int32_t world, mh_comm_t *comm_out); /* collective: every rank, same id */
mh_status mh_comm_destroy(mh_comm_t comm);
mh_status mh_comm_size(mh_comm_t comm, int32_t *rank_out, int32_t *world_out); /* as the communicator itself counted them */
mh_status mh_comm_broadcast(mh_comm_t comm, void *device_buf, size_t bytes, int32_t root, void *stream); /* in place, asynchronous */
mh_status mh_comm_broadcast_host(mh_comm_t comm, void *host_buf, size_t bytes, int32_t root); /* staged through the device, synchronous */
/* local_rows: [hi - lo][row_bytes] of mh_shard_range(B_total, rank, world), device; all_rows_out: [B_total][row_bytes], device, on every
 * rank.  Asynchronous on `stream`.  Ragged shards travel as they are (one grouped operation, no padding). */
mh_status mh_comm_all_gather_rows(mh_comm_t comm, const void *local_rows, int64_t B_total, size_t row_bytes, void *all_rows_out, void *stream);
/* The operations mh_comm_all_gather_rows issues on `rank` of `world`, without issuing them (host-only: no RCCL, no device).  Step k is a
 * broadcast of `bytes` bytes from rank `root` into [recv_offset, recv_offset + bytes) of every rank's output, in place except on the root
 * (send_local = 1: the bytes come from its local rows); equal shards give ONE step with root = -1, the plain all-gather.  Every rank gets
 * the same list (roots, sizes, offsets, order).  steps may be NULL with cap = 0 to ask for the count only (at most world steps). */
typedef struct mh_gather_step
{
   int32_t root;
   int32_t send_local;
   int64_t recv_offset;
   int64_t bytes;
} mh_gather_step;
mh_status mh_comm_gather_plan(int64_t B_total, size_t row_bytes, int32_t rank, int32_t world, int32_t force_ragged, mh_gather_step *steps,
                              int32_t cap, int32_t *n_steps_out);
mh_status mh_comm_barrier(mh_comm_t comm, void *stream); /* every rank has arrived and `stream` has drained */

/* ---- measurement helper: HIP-event timing of launches on a stream (bench.py, §8d timing protocol) ---- */
typedef struct mh_timer *mh_timer_t;
mh_status mh_timer_create(mh_timer_t *timer_out);
void mh_timer_destroy(mh_timer_t timer);
mh_status mh_timer_start(mh_timer_t timer, void *stream);
mh_status mh_timer_stop(mh_timer_t timer, void *stream);
mh_status mh_timer_elapsed_ms(mh_timer_t timer, float *ms_out); /* synchronises on the stop event */

#ifdef __cplusplus
}
#endif
#endif /* MECANO_HIP_H */
