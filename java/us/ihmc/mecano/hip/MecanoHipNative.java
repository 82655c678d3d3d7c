package us.ihmc.mecano.hip;

import java.lang.foreign.Arena;
import java.lang.foreign.FunctionDescriptor;
import java.lang.foreign.Linker;
import java.lang.foreign.MemoryLayout;
import java.lang.foreign.MemorySegment;
import java.lang.foreign.StructLayout;
import java.lang.foreign.SymbolLookup;
import java.lang.invoke.MethodHandle;

import static java.lang.foreign.ValueLayout.ADDRESS;
import static java.lang.foreign.ValueLayout.JAVA_DOUBLE;
import static java.lang.foreign.ValueLayout.JAVA_INT;
import static java.lang.foreign.ValueLayout.JAVA_LONG;

/**
 * Panama (java.lang.foreign, JDK 22+) binding of include/mecano_hip.h, ABI version 5.  NOT compiled in this repository's image (no JVM
 * there); it is the reference-side stub a Mecano maintainer adds.  One downcall handle per C entry point the shim classes use; every
 * entry point returns an mh_status int which {@link #check(int)} maps back to the exception types Mecano itself throws.
 * <p>
 * Pointer arguments named "host" are heap / off-heap memory of the JVM; "device" pointers come from {@link #DEVICE_ALLOC}.
 */
public final class MecanoHipNative
{
   private static final Linker LINKER = Linker.nativeLinker();
   private static final SymbolLookup LIB = SymbolLookup.libraryLookup(System.getProperty("mecano.hip.library", "libmecano_hip.so"), Arena.global());

   private static MethodHandle handle(String name, FunctionDescriptor descriptor)
   {
      return LINKER.downcallHandle(LIB.find(name).orElseThrow(() -> new UnsatisfiedLinkError(name)), descriptor);
   }

   private static FunctionDescriptor status(MemoryLayout... arguments)
   {
      return FunctionDescriptor.of(JAVA_INT, arguments);
   }

   /** the ABI version this binding was written against (include/mecano_hip.h: MH_ABI_VERSION); checked when the class loads */
   static final int ABI = 5;

   /**
    * struct mh_options { int32 consider_coriolis, consider_accelerations, layout, use_root_acceleration; void *stream; double
    * root_acceleration[6]; void *context; }
    */
   static final StructLayout OPTIONS = MemoryLayout.structLayout(JAVA_INT.withName("consider_coriolis"), JAVA_INT.withName("consider_accelerations"),
                                                                JAVA_INT.withName("layout"), JAVA_INT.withName("use_root_acceleration"),
                                                                ADDRESS.withName("stream"), MemoryLayout.sequenceLayout(6, JAVA_DOUBLE).withName("root_acceleration"),
                                                                ADDRESS.withName("context"));

   static final MethodHandle ABI_VERSION = handle("mh_abi_version", FunctionDescriptor.of(JAVA_INT));
   static final MethodHandle LAST_ERROR = handle("mh_last_error", FunctionDescriptor.of(ADDRESS));
   static final MethodHandle MODEL_CREATE = handle("mh_model_create", status(ADDRESS, ADDRESS));
   static final MethodHandle MODEL_DESTROY = handle("mh_model_destroy", FunctionDescriptor.ofVoid(ADDRESS));
   static final MethodHandle MODEL_KERNEL_VARIANT = handle("mh_model_kernel_variant", FunctionDescriptor.of(ADDRESS, ADDRESS));
   /** MH_WARN_* bits: model classes in which the engine consciously departs from Mecano (include/mecano_hip.h). */
   static final MethodHandle MODEL_WARNINGS = handle("mh_model_warnings", FunctionDescriptor.of(JAVA_INT, ADDRESS));
   static final MethodHandle MODEL_WARNING_TEXT = handle("mh_model_warning_text", FunctionDescriptor.of(ADDRESS, ADDRESS));
   static final int WARN_NEAR_COORDINATE_AXIS = 1, WARN_TINY_COMPOSITE_MASS = 2;
   /** (desc, out_dir|NULL, path_out, path_cap): runs hipcc on the kernel sources next to the library; minutes; once per robot. */
   static final MethodHandle BUILD_CODE_OBJECT = handle("mh_build_code_object", status(ADDRESS, ADDRESS, ADDRESS, JAVA_LONG));
   static final MethodHandle RESERVE = handle("mh_reserve", status(ADDRESS, JAVA_LONG));
   /**
    * Contexts: the model handle is read-only and shared; what compute calls write besides their outputs (workspace, scratch, hand-off flags,
    * error word) belongs to a context, one per thread / stream, named in mh_options.context (HipDeviceBatch owns one).
    */
   static final MethodHandle CONTEXT_CREATE = handle("mh_context_create", status(ADDRESS, ADDRESS));
   static final MethodHandle CONTEXT_DESTROY = handle("mh_context_destroy", FunctionDescriptor.ofVoid(ADDRESS));
   static final MethodHandle CONTEXT_RESERVE = handle("mh_context_reserve", status(ADDRESS, JAVA_LONG));
   /** (model, context|NULL, stream|NULL): synchronises the stream and reports failures of asynchronous calls that only showed on the device */
   static final MethodHandle MODEL_CHECK = handle("mh_model_check", status(ADDRESS, ADDRESS, ADDRESS));
   static final MethodHandle SET_JOINT_SOURCE_MODES = handle("mh_model_set_joint_source_modes", status(ADDRESS, ADDRESS));

   /* (model, B, q, qd, qdd|tau, gravity[3] (host), f_ext|NULL, opts|NULL, out) */
   private static final FunctionDescriptor DYNAMICS = status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS);
   /* (model, B, q, qd, qdd|tau, gravity, f_ext|NULL, opts|NULL, out, out2, out3): bodies (tau|qdd, body_acc, body_twist) */
   private static final FunctionDescriptor DYNAMICS_3 = status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                               ADDRESS);
   /* (model, B, q, qd, qdd|tau, gravity, f_ext|NULL, opts|NULL, out, joint_wrench_out) */
   private static final FunctionDescriptor DYNAMICS_2 = status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS);
   /* (model, B, q, qd, qdd, tau, gravity, f_ext|NULL, opts|NULL, tau_out, qdd_out) */
   private static final FunctionDescriptor PAIR = status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS);

   // ---- host-pointer entry points: copy in (chunked, three streams), launch, copy out, synchronise
   static final MethodHandle RNEA_HOST = handle("mh_rnea_f64_host", DYNAMICS);
   static final MethodHandle ABA_HOST = handle("mh_aba_f64_host", DYNAMICS);
   static final MethodHandle RNEA_ABA_HOST = handle("mh_rnea_aba_f64_host", PAIR);
   static final MethodHandle CRBA_HOST = handle("mh_crba_f64_host", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS));
   /** CompositeRigidBodyMassMatrixCalculator with setEnableCoriolisMatrixCalculation(true): (model, B, q, qd, opts, H_out, C_out). */
   static final MethodHandle CRBA_CORIOLIS_HOST = handle("mh_crba_coriolis_f64_host", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * getCentroidalMomentumMatrix / getCentroidalConvectiveTermMatrix: (model, B, q, qd, frame[12] or NULL, frame_mode, opts, A_out, b_out,
    * com_out); frame = centroidalMomentumFrame.getTransformToDesiredFrame(rootBody.getBodyFixedFrame()) as R row-major + p, frame_mode 1
    * for a CenterOfMassReferenceFrame under it.
    */
   static final MethodHandle CENTROIDAL_HOST = handle("mh_centroidal_f64_host", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, ADDRESS,
                                                                                       ADDRESS, ADDRESS, ADDRESS));

   // ---- device-pointer entry points (asynchronous on opts->stream): what HipDeviceBatch drives
   static final MethodHandle RNEA = handle("mh_rnea_f64", DYNAMICS);
   static final MethodHandle ABA = handle("mh_aba_f64", DYNAMICS);
   static final MethodHandle RNEA_ABA = handle("mh_rnea_aba_f64", PAIR);
   /** the same in fp32 (float matrices on the device) */
   static final MethodHandle RNEA_ABA_F32 = handle("mh_rnea_aba_f32", PAIR);
   /** (model, B, q, qd, qdd, gravity, f_ext|NULL, opts|NULL, tau_out, H_out): inverse dynamics and the mass matrix of the same state, one launch */
   static final MethodHandle RNEA_CRBA = handle("mh_rnea_crba_f64", DYNAMICS_2);
   /** (model, B, q, qd, qdd, gravity, opts|NULL, first_moment_columns, Y_out): JointTorqueRegressorCalculator.compute for B configurations */
   static final MethodHandle REGRESSOR = handle("mh_regressor_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, ADDRESS));
   /** (model, B, q, qd, tau, qdd_in, gravity, f_ext, opts, qdd_out, tau_out) */
   static final MethodHandle ABA_LOCKED = handle("mh_aba_locked_f64", PAIR);
   static final MethodHandle RNEA_BODIES = handle("mh_rnea_bodies_f64", DYNAMICS_3);
   static final MethodHandle ABA_BODIES = handle("mh_aba_bodies_f64", DYNAMICS_3);
   static final MethodHandle RNEA_JOINT_WRENCHES = handle("mh_rnea_joint_wrenches_f64", DYNAMICS_2);
   static final MethodHandle ABA_JOINT_WRENCHES = handle("mh_aba_joint_wrenches_f64", DYNAMICS_2);
   /** (model, B, q, body_acc, body_twist|NULL, gravity, n_pairs, base_joints (host int[]), body_joints (host int[]), opts, out) */
   static final MethodHandle RELATIVE_ACCELERATION = handle("mh_relative_acceleration_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                   JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * MultiBodyGravityGradientCalculator.getTauMatrix / getTauGradientMatrix for B configurations: (model, B, q, gravity[3] (host),
    * f_ext|NULL, opts|NULL, tau_out|NULL, grad_out|NULL), grad_out [B][nv][nv] row-major; not both outputs NULL.
    */
   static final MethodHandle GRAVITY_GRADIENT = handle("mh_gravity_gradient_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 (float matrices on the device) */
   static final MethodHandle GRAVITY_GRADIENT_F32 = handle("mh_gravity_gradient_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * Derivatives of the inverse dynamics at a moving state for B states: (model, B, q, qd, qdd, gravity[3] (host), f_ext|NULL, opts|NULL,
    * tau_out|NULL, dtau_dq_out|NULL, dtau_dqd_out|NULL), matrices [B][nv][nv] row-major; not both matrices NULL.
    */
   static final MethodHandle RNEA_DERIVATIVES = handle("mh_rnea_derivatives_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                         ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 (float matrices on the device) */
   static final MethodHandle RNEA_DERIVATIVES_F32 = handle("mh_rnea_derivatives_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                             ADDRESS, ADDRESS, ADDRESS));
   /**
    * Derivatives of the forward dynamics: (model, B, q, qd, tau, gravity[3] (host), f_ext|NULL, opts|NULL, qdd_out|NULL, dqdd_dq_out|NULL,
    * dqdd_dqd_out|NULL, Hinv_out|NULL), matrices [B][nv][nv] row-major; not both derivative matrices NULL.
    */
   static final MethodHandle ABA_DERIVATIVES = handle("mh_aba_derivatives_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                       ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_DERIVATIVES_F32 = handle("mh_aba_derivatives_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * Reverse-mode gradients of the inverse dynamics for a cotangent u of the efforts: (model, B, q, qd, qdd, gravity[3] (host), f_ext|NULL, u,
    * opts|NULL, gq_out|NULL, gqd_out|NULL, gqdd_out|NULL), vectors [B][nv]; not all three NULL.
    */
   static final MethodHandle RNEA_VJP = handle("mh_rnea_vjp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                         ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle RNEA_VJP_F32 = handle("mh_rnea_vjp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                             ADDRESS, ADDRESS, ADDRESS));
   /**
    * Reverse-mode gradients of the forward dynamics for a cotangent w of qdd: (model, B, q, qd, tau, gravity[3] (host), f_ext|NULL, w, opts|NULL,
    * qdd_out|NULL, gq_out|NULL, gqd_out|NULL, gtau_out|NULL), vectors [B][nv]; not all three gradients NULL.
    */
   static final MethodHandle ABA_VJP = handle("mh_aba_vjp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                       ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_VJP_F32 = handle("mh_aba_vjp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** q_out = q (+) dq, the pure configuration step of the velocity-space derivatives: (model, B, q, dq, opts|NULL, q_out); q_out may be q. */
   static final MethodHandle CONFIGURATION_ADD = handle("mh_configuration_add_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle CONFIGURATION_ADD_F32 = handle("mh_configuration_add_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** The dq_out with q0 (+) dq_out = q1: (model, B, q0, q1, opts|NULL, dq_out). */
   static final MethodHandle CONFIGURATION_DIFFERENCE = handle("mh_configuration_difference_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle CONFIGURATION_DIFFERENCE_F32 = handle("mh_configuration_difference_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * Linearisation of the simulation step: (model, B, dt, q, qd, tau, gravity[3] (host), f_ext|NULL, opts|NULL, qdd_out|NULL, q_next|NULL,
    * qd_next|NULL, A_out|NULL, B_out|NULL), A [B][2 nv][2 nv], B [B][2 nv][nv] row-major; not both matrices NULL, q_next and qd_next together.
    */
   static final MethodHandle ABA_INTEGRATE_DERIVATIVES = handle("mh_aba_integrate_derivatives_f64", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_INTEGRATE_DERIVATIVES_F32 = handle("mh_aba_integrate_derivatives_f32", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                               ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * Reverse-mode gradients of the integrator: (model, B, dt, qd, qdd, gq_next|NULL, gqd_next|NULL, opts|NULL, gq_out|NULL, gqd_out|NULL,
    * gqdd_out|NULL), vectors [B][nv]; not both cotangents NULL, not all three gradients NULL.
    */
   static final MethodHandle INTEGRATE_VJP = handle("mh_integrate_vjp_f64", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                   ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle INTEGRATE_VJP_F32 = handle("mh_integrate_vjp_f32", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                       ADDRESS, ADDRESS, ADDRESS));
   /**
    * Reverse-mode gradients of the simulation step: (model, B, dt, q, qd, tau, gravity[3] (host), f_ext|NULL, gq_next|NULL, gqd_next|NULL,
    * opts|NULL, qdd_out|NULL, gq_out|NULL, gqd_out|NULL, gtau_out|NULL), vectors [B][nv]; not both cotangents NULL, not all three gradients NULL.
    */
   static final MethodHandle ABA_INTEGRATE_VJP = handle("mh_aba_integrate_vjp_f64", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_INTEGRATE_VJP_F32 = handle("mh_aba_integrate_vjp_f32", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                               ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * Forward-mode derivatives of the inverse dynamics: (model, B, q, qd, qdd, gravity[3] (host), f_ext|NULL, dq|NULL, dqd|NULL, dqdd|NULL,
    * opts|NULL, dtau_out), vectors [B][nv]; not all three directions NULL.
    */
   static final MethodHandle RNEA_JVP = handle("mh_rnea_jvp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                         ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle RNEA_JVP_F32 = handle("mh_rnea_jvp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                             ADDRESS, ADDRESS));
   /**
    * Forward-mode derivatives of the forward dynamics: (model, B, q, qd, tau, gravity[3] (host), f_ext|NULL, dq|NULL, dqd|NULL, dtau|NULL,
    * opts|NULL, qdd_out|NULL, dqdd_out), vectors [B][nv]; not all three directions NULL.
    */
   static final MethodHandle ABA_JVP = handle("mh_aba_jvp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                       ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_JVP_F32 = handle("mh_aba_jvp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                           ADDRESS, ADDRESS, ADDRESS));
   /**
    * Forward-mode derivatives of the integrator: (model, B, dt, qd, qdd, dq|NULL, dqd|NULL, dqdd|NULL, opts|NULL, dq_next_out|NULL,
    * dqd_next_out|NULL), vectors [B][nv]; not all three directions NULL, not both outputs NULL.
    */
   static final MethodHandle INTEGRATE_JVP = handle("mh_integrate_jvp_f64", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                   ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle INTEGRATE_JVP_F32 = handle("mh_integrate_jvp_f32", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                       ADDRESS, ADDRESS, ADDRESS));
   /**
    * Forward-mode derivatives of the simulation step: (model, B, dt, q, qd, tau, gravity[3] (host), f_ext|NULL, dq|NULL, dqd|NULL, dtau|NULL,
    * opts|NULL, qdd_out|NULL, dqdd_out|NULL, dq_next_out|NULL, dqd_next_out|NULL), vectors [B][nv]; not all three directions NULL, not all
    * three tangents NULL.
    */
   static final MethodHandle ABA_INTEGRATE_JVP = handle("mh_aba_integrate_jvp_f64", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_INTEGRATE_JVP_F32 = handle("mh_aba_integrate_jvp_f32", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                               ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** The model's own inertial parameters: (model, pi_out (host double[n_joints][10])), the layout of a row of pi below. */
   static final MethodHandle MODEL_INERTIAL_PARAMETERS = handle("mh_model_inertial_parameters", status(ADDRESS, ADDRESS));
   /**
    * Inverse dynamics with per-configuration inertial parameters: (model, B, q, qd, qdd, pi, gravity[3] (host), f_ext|NULL, opts|NULL,
    * tau_out), pi [B][n_joints][10] on the device: (mass, com, Jxx, Jxy, Jxz, Jyy, Jyz, Jzz) per joint in description order.
    */
   static final MethodHandle RNEA_PARAMETERS = handle("mh_rnea_parameters_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                       ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle RNEA_PARAMETERS_F32 = handle("mh_rnea_parameters_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                           ADDRESS, ADDRESS));
   /** Forward dynamics with per-configuration inertial parameters: (model, B, q, qd, tau, pi, gravity[3] (host), f_ext|NULL, opts|NULL, qdd_out). */
   static final MethodHandle ABA_PARAMETERS = handle("mh_aba_parameters_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                     ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_PARAMETERS_F32 = handle("mh_aba_parameters_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                         ADDRESS, ADDRESS));
   /**
    * Reverse-mode gradient of the inverse dynamics with respect to the per-configuration inertial parameters, for a cotangent u of the
    * efforts: (model, B, q, qd, qdd, pi, gravity[3] (host), u, opts|NULL, gpi_out), gpi_out laid out like pi.
    */
   static final MethodHandle RNEA_PARAMETERS_VJP = handle("mh_rnea_parameters_vjp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                               ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle RNEA_PARAMETERS_VJP_F32 = handle("mh_rnea_parameters_vjp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                   ADDRESS, ADDRESS));
   /**
    * The same of the forward dynamics, for a cotangent w of qdd: (model, B, q, qd, tau, pi, gravity[3] (host), f_ext|NULL, w, opts|NULL,
    * qdd_out|NULL, gtau_out|NULL, gpi_out), gtau_out = H(pi)^-1 w.
    */
   static final MethodHandle ABA_PARAMETERS_VJP = handle("mh_aba_parameters_vjp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                             ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_PARAMETERS_VJP_F32 = handle("mh_aba_parameters_vjp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                 ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * Reverse-mode gradients of the inverse dynamics at per-configuration inertial parameters with respect to the state AND the parameters,
    * one launch: (model, B, q, qd, qdd, pi, gravity[3] (host), f_ext|NULL, u, opts|NULL, gq_out|NULL, gqd_out|NULL, gqdd_out|NULL,
    * gpi_out|NULL), not all four NULL; gpi_out laid out like pi, gqdd_out = H(pi) u.
    */
   static final MethodHandle RNEA_PARAMETERS_STATE_VJP = handle("mh_rnea_parameters_state_vjp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle RNEA_PARAMETERS_STATE_VJP_F32 = handle("mh_rnea_parameters_state_vjp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                               ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * The same of the forward dynamics, for a cotangent w of qdd: (model, B, q, qd, tau, pi, gravity[3] (host), f_ext|NULL, w, opts|NULL,
    * qdd_out|NULL, gq_out|NULL, gqd_out|NULL, gtau_out|NULL, gpi_out|NULL), not all four gradients NULL; gtau_out = H(pi)^-1 w.
    */
   static final MethodHandle ABA_PARAMETERS_STATE_VJP = handle("mh_aba_parameters_state_vjp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                         ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle ABA_PARAMETERS_STATE_VJP_F32 = handle("mh_aba_parameters_state_vjp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                                             ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** mh_apparent_inertia_inverse_*: the targets' own 6 x 6 blocks, or the coupled 6K x 6K matrix; at most this many targets per call */
   static final int APPARENT_BLOCKS_DIAGONAL = 0, APPARENT_BLOCKS_COUPLED = 1;
   static final int MAX_APPARENT_TARGETS = 16;
   /**
    * MultiBodyResponseCalculator.computeRigidBodyApparentSpatialInertiaInverse / applyRigidBodyWrench + getAccelerationChangeProvider for
    * B configurations and up to 16 target bodies, one launch: (model, B, q, n_targets, target_joints (host int[]), target_poses (host
    * double[n_targets][12])|NULL, blocks, opts|NULL, W_out), W_out [B][n_targets][6][6] or [B][6 n_targets][6 n_targets] row-major.
    */
   static final MethodHandle APPARENT_INERTIA_INVERSE = handle("mh_apparent_inertia_inverse_f64", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS,
                                                                                                           JAVA_INT, ADDRESS, ADDRESS));
   /** the same in fp32 (float q / W_out on the device; the poses stay double) */
   static final MethodHandle APPARENT_INERTIA_INVERSE_F32 = handle("mh_apparent_inertia_inverse_f32", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS,
                                                                                                               JAVA_INT, ADDRESS, ADDRESS));
   /** mh_body_poses_* / mh_geometric_jacobian_*: at most this many listed targets per call */
   static final int MAX_KINEMATIC_TARGETS = 16;
   /**
    * Poses of frames fixed in bodies, in the root body frame, for B configurations, one launch: (model, B, q, n_targets, target_joints (host
    * int[], -1 = the root body)|NULL = every body, target_poses (host double[n_targets][12])|NULL, opts|NULL, pose_out), pose_out
    * [B][n_targets][12], R row-major then p.
    */
   static final MethodHandle BODY_POSES = handle("mh_body_poses_f64", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 (float q / pose_out on the device; the poses stay double) */
   static final MethodHandle BODY_POSES_F32 = handle("mh_body_poses_f32", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * GeometricJacobianCalculator.getJacobianMatrix / getConvectiveTerm for B configurations and up to 16 kinematic chains, one launch:
    * (model, B, q, qd|NULL, n_targets, base_joints (host int[])|NULL = the root body, target_joints (host int[]), target_poses (host
    * double[n_targets][12])|NULL, opts|NULL, J_out, conv_out|NULL), J_out [B][6 n_targets][nv] row-major, conv_out [B][n_targets][6].
    */
   static final MethodHandle GEOMETRIC_JACOBIAN = handle("mh_geometric_jacobian_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS,
                                                                                               ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 (float q / qd / J_out / conv_out on the device; the poses stay double) */
   static final MethodHandle GEOMETRIC_JACOBIAN_F32 = handle("mh_geometric_jacobian_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS,
                                                                                                   ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /**
    * The gradient of a loss on body poses with respect to q for B configurations, one launch: (model, B, q, n_targets, target_joints (host
    * int[], -1 = the root body)|NULL = every body, target_poses (host double[n_targets][12])|NULL, g_pose, opts|NULL, gq_out), g_pose
    * [B][n_targets][12] the cotangent of BODY_POSES' pose_out, gq_out [B][nv] in the chart of mh_configuration_add.
    */
   static final MethodHandle BODY_POSES_VJP = handle("mh_body_poses_vjp_f64", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                       ADDRESS));
   /** the same in fp32 (float q / g_pose / gq_out on the device; the poses stay double) */
   static final MethodHandle BODY_POSES_VJP_F32 = handle("mh_body_poses_vjp_f32", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                           ADDRESS));
   /**
    * GeometricJacobianCalculator.getJointTorques summed over up to 16 kinematic chains without forming J, one launch: (model, B, q, n_targets,
    * base_joints (host int[])|NULL = the root body, target_joints (host int[]), target_poses (host double[n_targets][12])|NULL, wrench,
    * opts|NULL, tau_out), wrench [B][n_targets][6] (moment, force) in the target frames, tau_out [B][nv].
    */
   static final MethodHandle JACOBIAN_TRANSPOSE = handle("mh_jacobian_transpose_f64", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS,
                                                                                               ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 (float q / wrench / tau_out on the device; the poses stay double) */
   static final MethodHandle JACOBIAN_TRANSPOSE_F32 = handle("mh_jacobian_transpose_f32", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS,
                                                                                                   ADDRESS, ADDRESS, ADDRESS));
   /** mh_mass_matrix_inverse_*: at most this many listed columns per call */
   static final int MAX_INVERSE_COLUMNS = 64;
   /**
    * The inverse of the joint-space inertia matrix, or some of its columns, for B configurations, one launch: (model, B, q, n_columns,
    * columns (host int[])|NULL = all nv, opts|NULL, Hinv_out), Hinv_out [B][nv][nv] or [B][nv][n_columns] row-major, indexed like the mass
    * matrix.  MultiBodyResponseCalculator.computeJointApparentInertiaInverse is the joint's diagonal block.
    */
   static final MethodHandle MASS_MATRIX_INVERSE = handle("mh_mass_matrix_inverse_f64", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 (float q / Hinv_out on the device) */
   static final MethodHandle MASS_MATRIX_INVERSE_F32 = handle("mh_mass_matrix_inverse_f32", status(ADDRESS, JAVA_LONG, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS));
   /** mh_contact_impulse_*: at most this many contact points and sweeps per call */
   static final int MAX_CONTACT_TARGETS = 8, MAX_CONTACT_ITERATIONS = 4096;
   /**
    * The velocity after frictional point contacts have acted, for B configurations: (model, B, q, qd, n_targets, target_joints (host int[]),
    * target_poses (host double[n_targets][12])|NULL, mu (host double[n_targets]), normals|NULL, active|NULL, v_normal|NULL, impulse_init|NULL,
    * compliance, n_iterations, opts|NULL, qd_out, impulse_out|NULL, residual_out|NULL); normals [B][n_targets][3] in the root body frame,
    * active (int) and v_normal [B][n_targets], impulse_init / impulse_out [B][n_targets][6], residual_out [B].
    */
   static final MethodHandle CONTACT_IMPULSE = handle("mh_contact_impulse_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS,
                                                                                       ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_DOUBLE, JAVA_INT, ADDRESS, ADDRESS,
                                                                                       ADDRESS, ADDRESS));
   /** the same in fp32 (float state, normals, v_normal and impulses on the device; poses, mu and the compliance stay double) */
   static final MethodHandle CONTACT_IMPULSE_F32 = handle("mh_contact_impulse_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS,
                                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_DOUBLE, JAVA_INT, ADDRESS, ADDRESS,
                                                                                           ADDRESS, ADDRESS));
   /**
    * The same between two moving bodies: base_joints (host int[n_targets], -1 = the root body)|NULL behind target_joints; the impulse acts on the
    * target body and the base body receives its opposite at the same point.
    */
   static final MethodHandle CONTACT_IMPULSE_BETWEEN = handle("mh_contact_impulse_between_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS,
                                                                                                       ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_DOUBLE,
                                                                                                       JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   /** the same in fp32 */
   static final MethodHandle CONTACT_IMPULSE_BETWEEN_F32 = handle("mh_contact_impulse_between_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS,
                                                                                                           ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_DOUBLE,
                                                                                                           JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS));
   static final int MAX_LIMIT_JOINTS = 64, MAX_LIMIT_ITERATIONS = 4096;
   /**
    * The velocity after joint limits have acted, for B configurations: (model, B, q, qd, n_limits, limit_joints (host int[]), lower (host
    * double[n_limits]), upper (host double[n_limits]), margin, erp, impulse_init|NULL, compliance, n_iterations, opts|NULL, qd_out,
    * impulse_out|NULL, residual_out|NULL); impulse_init / impulse_out [B][n_limits], the generalised impulse on each listed joint, residual_out [B].
    */
   static final MethodHandle JOINT_LIMIT_IMPULSE = handle("mh_joint_limit_impulse_f64", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS,
                                                                                               JAVA_DOUBLE, JAVA_DOUBLE, ADDRESS, JAVA_DOUBLE, JAVA_INT, ADDRESS, ADDRESS,
                                                                                               ADDRESS, ADDRESS));
   /** the same in fp32 (float state and impulses on the device; the limits, margin, erp and the compliance stay double) */
   static final MethodHandle JOINT_LIMIT_IMPULSE_F32 = handle("mh_joint_limit_impulse_f32", status(ADDRESS, JAVA_LONG, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS,
                                                                                                   JAVA_DOUBLE, JAVA_DOUBLE, ADDRESS, JAVA_DOUBLE, JAVA_INT, ADDRESS, ADDRESS,
                                                                                                   ADDRESS, ADDRESS));
   /** (model, B, dt, q, qd, qdd, opts, q_out, qd_out, qdd_out|NULL) */
   static final MethodHandle INTEGRATE = handle("mh_integrate_f64", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                           ADDRESS));
   /** one simulation step: (model, B, dt, q, qd, tau, gravity, f_ext, opts, qdd_out, q_next, qd_next); q_next / qd_next may alias q / qd */
   static final MethodHandle ABA_INTEGRATE = handle("mh_aba_integrate_f64", status(ADDRESS, JAVA_LONG, JAVA_DOUBLE, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS,
                                                                                   ADDRESS, ADDRESS, ADDRESS, ADDRESS));

   // ---- memory: pinned host memory for PCIe-rate copies, device memory for state that stays resident
   static final MethodHandle HOST_ALLOC = handle("mh_host_alloc", status(JAVA_LONG, ADDRESS));
   static final MethodHandle HOST_FREE = handle("mh_host_free", status(ADDRESS));
   static final MethodHandle DEVICE_ALLOC = handle("mh_device_alloc", status(JAVA_LONG, ADDRESS));
   static final MethodHandle DEVICE_FREE = handle("mh_device_free", status(ADDRESS));
   static final MethodHandle COPY_TO_DEVICE = handle("mh_copy_to_device", status(ADDRESS, ADDRESS, JAVA_LONG, ADDRESS));
   static final MethodHandle COPY_TO_HOST = handle("mh_copy_to_host", status(ADDRESS, ADDRESS, JAVA_LONG, ADDRESS));
   static final MethodHandle STREAM_SYNCHRONIZE = handle("mh_stream_synchronize", status(ADDRESS));

   // ---- multi-GPU: one JVM per GPU, the batch sharded by rows, RCCL over xGMI (HipCommunicator)
   static final int COMM_ID_BYTES = 128;
   static final MethodHandle SET_DEVICE = handle("mh_set_device", status(JAVA_INT));
   static final MethodHandle SHARD_RANGE = handle("mh_shard_range", status(JAVA_LONG, JAVA_INT, JAVA_INT, ADDRESS, ADDRESS));
   static final MethodHandle COMM_UNIQUE_ID = handle("mh_comm_unique_id", status(ADDRESS));
   static final MethodHandle COMM_CREATE = handle("mh_comm_create", status(ADDRESS, JAVA_INT, JAVA_INT, ADDRESS));
   static final MethodHandle COMM_DESTROY = handle("mh_comm_destroy", status(ADDRESS));
   static final MethodHandle COMM_SIZE = handle("mh_comm_size", status(ADDRESS, ADDRESS, ADDRESS));
   static final MethodHandle COMM_BROADCAST = handle("mh_comm_broadcast", status(ADDRESS, ADDRESS, JAVA_LONG, JAVA_INT, ADDRESS));
   static final MethodHandle COMM_BROADCAST_HOST = handle("mh_comm_broadcast_host", status(ADDRESS, ADDRESS, JAVA_LONG, JAVA_INT));
   static final MethodHandle COMM_ALL_GATHER_ROWS = handle("mh_comm_all_gather_rows", status(ADDRESS, ADDRESS, JAVA_LONG, JAVA_LONG, ADDRESS, ADDRESS));
   static final MethodHandle COMM_BARRIER = handle("mh_comm_barrier", status(ADDRESS, ADDRESS));

   /** An mh_options in `arena`: the calculators' switches, AoS layout (rows = configurations), the null stream, gravity as the root acceleration. */
   static MemorySegment options(Arena arena, boolean considerCoriolis, boolean considerAccelerations)
   {
      return options(arena, considerCoriolis, considerAccelerations, null);
   }

   /**
    * The same with an explicit root acceleration (setRootAcceleration(SpatialAccelerationReadOnly), InverseDynamicsCalculator.java:413-427):
    * six doubles (angular, linear) in root-body coordinates, or null for "the call's gravity argument as (0, -g)".
    */
   static MemorySegment options(Arena arena, boolean considerCoriolis, boolean considerAccelerations, double[] rootAcceleration)
   {
      return options(arena, considerCoriolis, considerAccelerations, rootAcceleration, MemorySegment.NULL);
   }

   /** The same for calls made through a context (HipDeviceBatch.context); MemorySegment.NULL is the model's default context. */
   static MemorySegment options(Arena arena, boolean considerCoriolis, boolean considerAccelerations, double[] rootAcceleration, MemorySegment context)
   {
      MemorySegment options = arena.allocate(OPTIONS);
      options.set(JAVA_INT, 0, considerCoriolis ? 1 : 0);
      options.set(JAVA_INT, 4, considerAccelerations ? 1 : 0);
      options.set(JAVA_INT, 8, 0);
      options.set(JAVA_INT, 12, rootAcceleration == null ? 0 : 1);
      options.set(ADDRESS, 16, MemorySegment.NULL);
      for (int k = 0; k < 6; k++)
         options.set(JAVA_DOUBLE, 24 + 8L * k, rootAcceleration == null ? 0.0 : rootAcceleration[k]);
      options.set(ADDRESS, 72, context);
      return options;
   }

   static
   {
      int version;
      try
      {
         version = (int) ABI_VERSION.invokeExact();
      }
      catch (Throwable t)
      {
         throw new ExceptionInInitializerError(t);
      }
      if (version != ABI)
         throw new UnsatisfiedLinkError("libmecano_hip.so reports ABI version " + version + ", this binding was written for " + ABI);
   }

   /** mh_status -> the exception Mecano's own calculators would have thrown (SURVEY.md section 8b, "Errors"). */
   static void check(int status)
   {
      if (status == 0)
         return;
      String message;
      try
      {
         message = ((MemorySegment) LAST_ERROR.invokeExact()).reinterpret(512).getString(0);
      }
      catch (Throwable t)
      {
         message = "mh_status " + status;
      }
      switch (status)
      {
         case 1: // MH_ERR_INVALID_ARGUMENT
         case 5: // MH_ERR_BAD_TOPOLOGY
         case 6: // MH_ERR_BAD_AXIS
            throw new IllegalArgumentException(message);
         case 2: // MH_ERR_BAD_DIMENSION  (ForwardDynamicsCalculator.java:522-533)
            throw new org.ejml.MatrixDimensionException(message);
         case 3: // MH_ERR_UNSUPPORTED_JOINT
         case 4: // MH_ERR_LOOP_CLOSURE   (ForwardDynamicsCalculator.java:207-211 prints and skips; here it is explicit)
            throw new UnsupportedOperationException(message);
         case 9: // MH_ERR_OUT_OF_MEMORY
            throw new OutOfMemoryError(message);
         default: // MH_ERR_NO_DEVICE, MH_ERR_HIP, ...
            throw new IllegalStateException(message);
      }
   }

   /** Runs a downcall that returns an mh_status and converts checked Throwables (MethodHandle.invoke) into unchecked ones. */
   interface Call
   {
      int run() throws Throwable;
   }

   static void invoke(Call call)
   {
      int status;
      try
      {
         status = call.run();
      }
      catch (RuntimeException | Error e)
      {
         throw e;
      }
      catch (Throwable t)
      {
         throw new IllegalStateException(t);
      }
      check(status);
   }

   private MecanoHipNative()
   {
   }
}
