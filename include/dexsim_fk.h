/* dexsim_fk.h -- the forward-kinematics entry point of libdexsim's C-ABI.  A part of include/dexsim.h, which includes this file
 * inside its extern "C" block behind the types it needs (dexsim_t, <stdint.h>): include dexsim.h, not this file.
 * dexrobot_isaac_amd/_abi.py mirrors it as FK_PROTOTYPES, next to PROTOTYPES for the declarations written in dexsim.h itself. */
#ifndef DEXSIM_FK_H
#define DEXSIM_FK_H

/* ------------------------------------------------------------------ forward kinematics: body states, site poses, centroid
 * The configuration the other queries describe: where the hand bodies and the fingertips are for a batch of joint positions, how
 * they move, and where the hand's centre of mass is -- for sampling planners (MPPI, CEM), IK loops (where did the tips end up?),
 * reachability sweeps and rewards on candidate configurations; with dexsim_solve_ik, dexsim_query_proximity and
 * dexsim_body_jacobian at the same rows it composes IK -> FK -> clearance -> Jacobian.  dexsim_refresh_body_states is the same
 * kinematics for the envs' own state into the bound API tensor; this call has row selection, body selection and overrides.  One
 * launch, stream-ordered, never synchronises, allocates nothing; it writes no arena word, API tensor, statistics word, counter or
 * the step stamp.  A row's result depends on that row alone and is reproducible bit for bit.
 *
 * ROWS and the Q OVERRIDE are those of dexsim_body_jacobian: with q == NULL row i is env env_ids[i] (NULL: env i, k == num_envs)
 * with its current q and qd (arena), qd must be NULL, and a row whose id is outside [0, num_envs) leaves all its output rows
 * untouched; with q != NULL, a device (k, 26) array, env_ids is ignored and k may be any positive number.  VELOCITIES with a q
 * override: qd is an OPTIONAL device (k, 26) override; with qd == NULL every velocity word and the kinetic energy are exact +0.0f.
 * This is the one deliberate difference from dexsim_inverse_dynamics, where q and qd go together: poses need no velocities, and a
 * planner should not have to allocate zeros.  An override row equal to an env's (q, qd) gives that env's state-path bits.
 *
 * OUTPUTS, f32; any of the three may be NULL, not all.
 * body_states (k, nb, 13), 4-byte aligned: layout and meaning of a rigid_body_states row -- words 0-2 position of the body-frame
 *   origin, 3-6 quaternion xyzw = frame (x) body_q[b], 7-9 world linear velocity of that origin, 10-12 world angular velocity.
 *   bodies / nb as for dexsim_body_jacobian: a HOST array of nb hand-body indices, NULL = all DEXSIM_NUM_HAND_BODIES in order, nb
 *   must then be DEXSIM_NUM_HAND_BODIES, and a model whose body_parent differs from the frames rigid_body_states is published on is
 *   refused.  They are ignored (may be NULL / 0) when body_states is NULL.  Body 0 (hand_mount) has the spawn pose and a twist of exact +0.0f.
 *   Contract: jac[i, b] @ qd of dexsim_body_jacobian is words 7-12.
 * site_poses (k, DEXSIM_NSITE, 7), 4-byte aligned: position and quaternion xyzw of the sites in model order (right_hand_base, five
 *   tips, five pads).  flags == 0: in the env's world frame, as the obs key fingertip_poses_world has the tips.  With
 *   DEXSIM_FK_HAND_FRAME: relative to site 0 by the rule of the observation stage, p_h = R(q_0)^T (p - p_0), q_h = conj(q_0) (x) q --
 *   what fingertip_poses_hand / fingerpad_poses_hand hold; site 0 itself is then (0, 0, 0, 0, 0, 0, 1) up to rounding.
 * centroid (k, 8), 16-byte aligned, over the 26 links with the mass, com and inertia of DexHandModel (general symmetric tensors):
 *     0-2   centre of mass of the hand, world frame
 *     3     potential energy -sum_j m_j g . c_j for cfg.gravity: zero at the env's world origin
 *     4-6   velocity of the centre of mass
 *     7     kinetic energy sum_j 1/2 m_j |v_cj|^2 + 1/2 w_j^T I_j w_j = 1/2 qd^T M(q) qd with the M of dexsim_mass_matrix
 *   The sums run in one fixed order (fingers 0..4, then the base links) about the palm joint's origin and are shifted to the world
 *   once.  Contract: gravity . qd of dexsim_mass_matrix is -M_tot g . (words 4-6).
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed, nothing is launched): NULL handle, k <= 0, env_ids == NULL
 * without q and k != num_envs, qd without q, all three outputs NULL, with body_states a bad body list (nb outside
 * [1, DEXSIM_NUM_HAND_BODIES], an index out of range, bodies == NULL with nb != DEXSIM_NUM_HAND_BODIES), an unknown flag bit, a
 * misaligned output.  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
#define DEXSIM_FK_HAND_FRAME 1   /* site_poses relative to site 0 (right_hand_base) */
int dexsim_forward_kinematics(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const int* bodies, int nb,
                              int flags, float* body_states, float* site_poses, float* centroid, void* stream);

#endif /* DEXSIM_FK_H */
