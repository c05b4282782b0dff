/* dexsim_ray.h -- the range-sensor entry point of libdexsim's C-ABI.  A part of include/dexsim.h, which includes this file inside
 * its extern "C" block behind the camera sensors, whose segment ids and intersection rule it uses: include dexsim.h, not this file.
 * dexrobot_isaac_amd/_abi.py mirrors it as RAY_PROTOTYPES, next to PROTOTYPES for the declarations written in dexsim.h itself. */
#ifndef DEXSIM_RAY_H
#define DEXSIM_RAY_H

/* ------------------------------------------------------------------ range sensors: batched ray casts with distance, hit and normal
 * Time-of-flight and proximity sensors in the fingertips, a range array on the palm, a lidar fan beside the table, a line-of-sight
 * test between two points: a few dozen arbitrary rays, each mounted on a frame of the hand or on the env's world frame, read every
 * control step as a small (k, nrays) tensor -- MuJoCo's rangefinder, Isaac Lab's RayCaster.  A camera casts a pinhole fan from one
 * eye and returns images; this call casts any list of rays and returns records.  One launch, no workspace, stream-ordered, never
 * synchronises, allocates nothing; a pure function of the persistent state (arena fields q, box_pos, box_quat) or of the caller's
 * overrides: it writes no arena word, API tensor, statistics word, counter or the step stamp.
 *
 * ROWS, the Q OVERRIDE and THE BOX are those of dexsim_query_proximity: with q == NULL row i is env env_ids[i] (NULL: env i,
 * k == num_envs) and a row whose id is outside [0, num_envs) leaves its output rows untouched; with q != NULL, a device (k, 26) array,
 * env_ids is ignored and k may be any positive number.  The box of a row is box_pose, a device (k, 7) f32 array (centre xyz,
 * quaternion xyzw, normalised by the call), when it is given; otherwise the row's env's own box when q == NULL and cfg.has_box;
 * otherwise there is none.  Edge length: box_size if it is > 0, else cfg.box_size.  A row's result depends on that row alone and is
 * reproducible bit for bit; a q / box_pose row equal to an env's state gives that env's output bit for bit, and a ray of a long list
 * gives the bits of the same ray cast alone.
 *
 * RAYS.  rays: a DEVICE (nrays, 6) f32 array shared by all rows -- origin xyz and direction xyz in the ray's parent frame.  The
 * direction is normalised by the call; a direction with |d|^2 < 1e-24 (or not finite) never hits.  parent: a HOST array of nrays
 * ints, like the bodies of the Jacobian call: -1 is the env's world frame, 0 .. DEXSIM_NJ - 1 that joint's frame, the parent_joint
 * convention of DexSimCamera (5 = the palm joint; the tip and pad sites ride on joint 9 + 4 f).  parent must be NON-DECREASING:
 * sort the rays by parent.
 *
 * INTERSECTION: the rule of the camera sensors (dexsim.h, PIXEL MODEL), restated here so that the two cannot drift.  Every primitive contributes the point where the ray ENTERS it (a ray that
 * starts inside a primitive does not see it; the ground is hit from either side).  Ground: the plane z = 0, two-sided.  Box: the
 * cube, its entering slab hit only.  Capsule: the union of the open cylinder and the two end spheres, the entering hit only.  t is
 * the distance in metres along the unit direction.  A hit counts when min_range <= t <= max_range; the nearest hit wins; on a tie
 * the earlier shape wins, in the order ground, box, capsule 0 .. DEXSIM_NCAP - 1.  With DEXSIM_RAY_SKIP_PARENT in flags a ray
 * mounted on joint frame j >= 0 does not test the capsules with cap_parent == j: a sensor inside its own link's skin looks out.
 *
 * OUTPUTS, f32, 16-byte aligned; either may be NULL, not both.
 *   dist (k, nrays)      t of the hit, +inf without one
 *   hits (k, nrays, 8)   word 0 t; words 1-3 the hit point; words 4-6 the outward unit normal of the surface at the hit (the ground:
 *                        +z from either side); word 7 the integer bits of the int32 segment id DEXSIM_SEG_NONE, DEXSIM_SEG_GROUND,
 *                        DEXSIM_SEG_BOX or DEXSIM_SEG_CAPSULE0 + c.  Point and normal are in the env's world frame, the
 *                        frame of rigid_body_states.  Without a hit the record is +inf, six words +0.0f and DEXSIM_SEG_NONE.
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed, nothing is launched): nrays outside [1, DEXSIM_RAY_MAX], NULL rays or
 * parent, a parent outside [-1, DEXSIM_NJ) or a decreasing parent list, a range that is not finite, min_range < 0 or
 * min_range >= max_range, flag bits other than DEXSIM_RAY_SKIP_PARENT, both outputs NULL or a misaligned output, a non-finite
 * box_size, k <= 0, a NULL handle, env_ids == NULL without q and k != num_envs, with DEXSIM_RAY_SKIP_PARENT a model whose cap_parent
 * is outside [0, DEXSIM_NJ), a box without a positive edge length.  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
#define DEXSIM_RAY_MAX          4096   /* rays per call */
#define DEXSIM_RAY_SKIP_PARENT  1      /* flag: a ray mounted on joint frame j >= 0 does not test the capsules with cap_parent == j */
int dexsim_raycast(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* box_pose, float box_size,
                   const float* rays, const int* parent, int nrays, float min_range, float max_range, int flags,
                   float* dist, float* hits, void* stream);

#endif /* DEXSIM_RAY_H */
