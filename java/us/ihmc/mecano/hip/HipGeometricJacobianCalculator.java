package us.ihmc.mecano.hip;

import java.lang.foreign.Arena;
import java.lang.foreign.MemorySegment;
import java.util.ArrayList;
import java.util.List;

import org.ejml.data.DMatrixRMaj;

import us.ihmc.mecano.multiBodySystem.interfaces.JointReadOnly;
import us.ihmc.mecano.multiBodySystem.interfaces.MultiBodySystemReadOnly;
import us.ihmc.mecano.multiBodySystem.interfaces.RigidBodyReadOnly;
import us.ihmc.mecano.tools.MultiBodySystemTools;

import static java.lang.foreign.ValueLayout.ADDRESS;
import static java.lang.foreign.ValueLayout.JAVA_DOUBLE;
import static java.lang.foreign.ValueLayout.JAVA_INT;

/**
 * Batched drop-in for GeometricJacobianCalculator (java:103-158, 232-279, 316-377, 440-633): the geometric Jacobian of the kinematic chain
 * from a base to an end effector -- any two bodies of the system, the chain may cross their common ancestor (java:258-277) -- and its
 * convective term, for B configurations at once, one launch of mh_geometric_jacobian_f64 per reset.
 * <p>
 * reset(q, qd) sets the B states (one ROW each; the reference reads them from the joints' frames; qd may be null while the convective
 * term is not asked for).  Matrices are B x (6 * dofs), row b = the reference's 6 x dofs matrix (row-major) with the columns in
 * base-to-end-effector joint order (java:260-277).  The Jacobian frame is the end effector's body-fixed frame, or a frame fixed in the
 * end effector given as a pose (12 numbers, R row-major then p) relative to it: the only case in which the reference's convective term
 * is valid (its warning, java:288, 587, 605).
 * </p>
 * Source only: this image has no JDK (INTEGRATION.md).
 */
public class HipGeometricJacobianCalculator implements AutoCloseable
{
   private final MultiBodySystemReadOnly input;
   private final HipMultiBodyModel model;
   private HipDeviceBatch batch;
   private boolean hasVelocities;
   private RigidBodyReadOnly base, endEffector;
   private double[] jacobianFramePose;
   private final List<JointReadOnly> jointsFromBaseToEndEffector = new ArrayList<>(12);
   private int[] chainColumns = new int[0];
   private boolean jacobianUpToDate, convectiveTermUpToDate;
   private final DMatrixRMaj jacobianMatrix = new DMatrixRMaj(0, 0), convectiveTerm = new DMatrixRMaj(0, 0);

   public HipGeometricJacobianCalculator(MultiBodySystemReadOnly input)
   {
      this.input = input;
      model = new HipMultiBodyModel(input);
   }

   /** java:127-131 plus the states: q is B x nq, qd B x nv or null. */
   public void reset(DMatrixRMaj q, DMatrixRMaj qd)
   {
      int B = q.getNumRows();
      if (q.getNumCols() != model.nq || (qd != null && (qd.getNumRows() != B || qd.getNumCols() != model.nv)))
         throw new org.ejml.MatrixDimensionException("Expected q: B x " + model.nq + ", qd: B x " + model.nv);
      if (batch == null || batch.batchSize != B)
      {
         if (batch != null)
            batch.close();
         batch = new HipDeviceBatch(model, B);
      }
      batch.setConfiguration(q);
      hasVelocities = qd != null;
      if (hasVelocities)
         batch.setVelocity(qd);
      jacobianUpToDate = convectiveTermUpToDate = false;
   }

   /** java:148-158; the Jacobian frame goes back to the end effector's body-fixed frame. */
   public void setKinematicChain(RigidBodyReadOnly base, RigidBodyReadOnly endEffector)
   {
      if (indexOf(base) < -1 || indexOf(endEffector) < -1)
         throw new IllegalArgumentException("Base and end-effector must be bodies this calculator's system considers.");
      this.base = base;
      this.endEffector = endEffector;
      jacobianFramePose = null;
      MultiBodySystemTools.collectJointPath(base, endEffector, jointsFromBaseToEndEffector);
      int dofs = 0;
      for (JointReadOnly joint : jointsFromBaseToEndEffector)
         dofs += joint.getDegreesOfFreedom();
      chainColumns = new int[dofs];
      int column = 0;
      for (JointReadOnly joint : jointsFromBaseToEndEffector)
         for (int index : input.getJointMatrixIndexProvider().getJointDoFIndices(joint))
            chainColumns[column++] = index;
      jacobianUpToDate = convectiveTermUpToDate = false;
   }

   /**
    * java:232-238, for a frame fixed in the end effector only: its pose relative to the end effector's body-fixed frame (12 numbers, R
    * row-major then p), or null for the body-fixed frame itself.
    */
   public void setJacobianFrame(double[] poseInEndEffector)
   {
      if (poseInEndEffector != null && poseInEndEffector.length != 12)
         throw new IllegalArgumentException("A pose is 12 numbers: R row-major, then p.");
      jacobianFramePose = poseInEndEffector == null ? null : poseInEndEffector.clone();
      jacobianUpToDate = convectiveTermUpToDate = false;
   }

   /** position in the model's joint list of the body's parent joint; -1 for the root body, -2 for a body that is not considered */
   private int indexOf(RigidBodyReadOnly body)
   {
      if (body.getParentJoint() == null)
         return body == input.getRootBody() ? -1 : -2;
      int index = model.indexOf(body.getParentJoint());
      return index < 0 ? -2 : index;
   }

   private void update(boolean withConvectiveTerm)
   {
      if (base == null || endEffector == null)
         throw new RuntimeException("The base and end-effector have to be set first."); // java:254-255
      if (batch == null)
         throw new RuntimeException("Call reset(q, qd) with the states first.");
      if (jacobianUpToDate && (convectiveTermUpToDate || !withConvectiveTerm))
         return;
      if (withConvectiveTerm && !hasVelocities)
         throw new RuntimeException("The convective term needs the velocities: reset(q, qd).");
      int B = batch.batchSize, nv = model.nv, dofs = chainColumns.length;
      long jCount = (long) B * 6 * nv, cCount = (long) B * 6;
      try (Arena arena = Arena.ofConfined())
      {
         MemorySegment result = arena.allocate(ADDRESS);
         MecanoHipNative.invoke(() -> (int) MecanoHipNative.DEVICE_ALLOC.invokeExact((jCount + cCount) * Double.BYTES, result));
         MemorySegment device = result.get(ADDRESS, 0);
         try
         {
            MemorySegment deviceJ = device;
            MemorySegment deviceC = withConvectiveTerm ? MemorySegment.ofAddress(device.address() + jCount * Double.BYTES) : MemorySegment.NULL;
            MemorySegment bases = arena.allocateFrom(JAVA_INT, new int[] {indexOf(base)}), targets = arena.allocateFrom(JAVA_INT, new int[] {indexOf(endEffector)});
            MemorySegment pose = jacobianFramePose == null ? MemorySegment.NULL : arena.allocateFrom(JAVA_DOUBLE, jacobianFramePose);
            MemorySegment velocities = withConvectiveTerm ? batch.qd : MemorySegment.NULL;
            MemorySegment options = MecanoHipNative.options(arena, true, true);
            MecanoHipNative.invoke(() -> (int) MecanoHipNative.GEOMETRIC_JACOBIAN.invokeExact(model.handle, (long) B, batch.q, velocities, 1, bases, targets, pose,
                                                                                             options, deviceJ, deviceC));
            long count = withConvectiveTerm ? jCount + cCount : jCount;
            MemorySegment host = arena.allocate(JAVA_DOUBLE, Math.max(1, count));
            if (count > 0)
               MecanoHipNative.invoke(() -> (int) MecanoHipNative.COPY_TO_HOST.invokeExact(host, device, count * Double.BYTES, MemorySegment.NULL));
            MecanoHipNative.invoke(() -> (int) MecanoHipNative.STREAM_SYNCHRONIZE.invokeExact(MemorySegment.NULL));
            jacobianMatrix.reshape(B, 6 * dofs);
            for (int b = 0; b < B; b++)
               for (int row = 0; row < 6; row++)
                  for (int c = 0; c < dofs; c++)
                     jacobianMatrix.set(b, row * dofs + c, host.getAtIndex(JAVA_DOUBLE, ((long) b * 6 + row) * nv + chainColumns[c]));
            if (withConvectiveTerm)
            {
               convectiveTerm.reshape(B, 6);
               for (int b = 0; b < B; b++)
                  for (int row = 0; row < 6; row++)
                     convectiveTerm.set(b, row, host.getAtIndex(JAVA_DOUBLE, jCount + (long) b * 6 + row));
            }
         }
         finally
         {
            MecanoHipNative.invoke(() -> (int) MecanoHipNative.DEVICE_FREE.invokeExact(device));
         }
      }
      jacobianUpToDate = true;
      convectiveTermUpToDate = withConvectiveTerm;
   }

   /** java:578-582: B x (6 * dofs) */
   public DMatrixRMaj getJacobianMatrix()
   {
      update(false);
      return jacobianMatrix;
   }

   /** java:611-615: B x 6, JDot * qDot */
   public DMatrixRMaj getConvectiveTermMatrix()
   {
      update(true);
      return convectiveTerm;
   }

   /** java:440-444: B x 6 = J * jointVelocities (B x dofs, starting from the base's child joint) */
   public DMatrixRMaj getEndEffectorTwist(DMatrixRMaj jointVelocities)
   {
      DMatrixRMaj J = getJacobianMatrix();
      int dofs = chainColumns.length;
      DMatrixRMaj out = new DMatrixRMaj(J.getNumRows(), 6);
      for (int b = 0; b < J.getNumRows(); b++)
         for (int row = 0; row < 6; row++)
         {
            double sum = 0.0;
            for (int c = 0; c < dofs; c++)
               sum += J.get(b, row * dofs + c) * jointVelocities.get(b, c);
            out.set(b, row, sum);
         }
      return out;
   }

   /** java:456-461: B x 6 = J * jointAccelerations + the convective term */
   public DMatrixRMaj getEndEffectorAcceleration(DMatrixRMaj jointAccelerations)
   {
      DMatrixRMaj out = getEndEffectorTwist(jointAccelerations), c = getConvectiveTermMatrix();
      for (int i = 0; i < out.getNumElements(); i++)
         out.data[i] += c.data[i];
      return out;
   }

   /** java:477-484: B x dofs = J^T * wrench, the wrench (moment, force; B x 6) on the end effector expressed in the Jacobian frame */
   public DMatrixRMaj getJointTorques(DMatrixRMaj endEffectorWrench)
   {
      DMatrixRMaj J = getJacobianMatrix();
      int dofs = chainColumns.length;
      DMatrixRMaj out = new DMatrixRMaj(J.getNumRows(), dofs);
      for (int b = 0; b < J.getNumRows(); b++)
         for (int c = 0; c < dofs; c++)
         {
            double sum = 0.0;
            for (int row = 0; row < 6; row++)
               sum += J.get(b, row * dofs + c) * endEffectorWrench.get(b, row);
            out.set(b, c, sum);
         }
      return out;
   }

   /** java:567-570 */
   public List<JointReadOnly> getJointsFromBaseToEndEffector()
   {
      return jointsFromBaseToEndEffector;
   }

   /** java:556-559 */
   public int getNumberOfDegreesOfFreedom()
   {
      return endEffector == null ? -1 : chainColumns.length;
   }

   public RigidBodyReadOnly getBase()
   {
      return base;
   }

   public RigidBodyReadOnly getEndEffector()
   {
      return endEffector;
   }

   @Override
   public void close()
   {
      if (batch != null)
         batch.close();
      model.close();
   }
}
