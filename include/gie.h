/*
 * gie.h — C-ABI of the MI355X-native incremental-EDT map-update path.
 *
 * This is the drop-in boundary for the per-frame hot path of JINXER000/GIE-mapping
 * (VOLMAPNODE::publishMap, src/volumetric_mapper.cpp:138-224).  The reference has no FFI
 * layer; its boundary is the set of C++ objects the ROS node calls.  Every entry point below
 * names the reference symbol it replaces (file:line relative to the reference tree).
 *
 * Conventions: opaque handle, int status codes (0 = GIE_OK), gie_last_error() for the text,
 * no exceptions cross the ABI, one handle is not thread-safe (the reference is single-threaded,
 * src/main.cpp:7), buffers are caller-owned HOST pointers unless the name ends in _dev.
 * All dense local-volume arrays are x-fastest: idx = z*X*Y + y*X + x (local_batch.h:394-407).
 */
#ifndef GIE_H
#define GIE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GIE_OK 0
#define GIE_ERR_INVALID 1   /* bad argument / bad call order            */
#define GIE_ERR_DEVICE 2    /* HIP runtime error                        */
#define GIE_ERR_CAPACITY 3  /* block pool / hash / frontier queue full  */
#define GIE_ERR_TIMEOUT 4   /* the wavefront kernel's grid barrier timed out: its workgroups were kept off the device for
                               seconds (another process's kernels holding the compute units).  The map update that hit it is
                               incomplete (waves cut short, distances may be over-estimates until the region is observed
                               again); the condition is reported once and cleared — the next update runs normally.  What the
                               incomplete update leaves in the map: Mark's own distances are committed (Mark and commit are one
                               sweep unless the changed-block flags are on — then nothing of that update is committed), what the
                               waves would have lowered or raised behind them is not.  One process per device is the supported
                               configuration. */

/* voxel types, local_batch.h:7-10 */
#define GIE_VOX_UNKNOWN 0
#define GIE_VOX_FREE 1
#define GIE_VOX_OCCUPIED 2
#define GIE_VOX_FNT 3

/* sentinels, voxmap_utils.cuh:8-9 */
#define GIE_EMPTY_VALUE 999999

typedef struct gie_mapper gie_mapper;

/* LocMap ctor arguments (local_batch.h:35-60) + the Parameters fields that reach the GPU code
 * (parameters.h:69-132) + GlbHashMap capacity (glb_hash_map.cu:9-47). */
typedef struct gie_config {
    float voxel_width;            /* m, Parameters::voxel_width                               */
    int32_t local_size[3];        /* voxels (X,Y,Z) = local_size_{x,y,z}/voxel_width           */
    int32_t occupancy_threshold;  /* 0..255, default 180                                       */
    float ogm_min_h, ogm_max_h;   /* height gate for occupied hits (ogm/min_height,max_height) */
    int32_t cutoff_grids_sq;      /* ceil(cutoff_dist/voxel_width)^2, parameters.h:95,134-138  */
    int32_t fast_mode;            /* wave/fast_mode (code default true, parameters.h:93)       */
    int32_t for_motion_planner;   /* robot sphere forced FREE in the OGM kernels               */
    int32_t robot_r2_grids;       /* ceil(robot_r/voxel_width)^2                               */
    int32_t max_blocks;           /* block pool capacity (hash/block_max); 0 = size from volume.  19.5 KB of device memory per block; voxel addresses are 64-bit, so the device's memory is the limit */
    int32_t device_id;            /* HIP device ordinal                                         */
    int32_t retain_radius_blocks; /* block-pool lifecycle.  0 = the reference's rule: blocks are never freed and the pool only
                                     shrinks (BlockAllocBase::allocate_n throws when it is empty, blockalloc.h:50-67; its free
                                     list, blockalloc.h:69-118, is never fed).  R > 0: at the start of every gie_fuse the
                                     blocks whose block coordinate lies more than R blocks (Chebyshev) outside the block box
                                     of the local volume +-1 voxel are erased — their voxels revert to the defaults
                                     (UNKNOWN, EMPTY_VALUE, EMPTY_KEY) — and go back to the pool's free list, so a robot
                                     that drives on forever runs on a fixed pool.  Erased blocks are not streamed. */
    int32_t wave_workgroups;      /* workgroups of the persistent wavefront kernel (waves A / B / C; its grid barrier needs all of them resident
                                     at once).  0 = half the device's compute units, so that two mappers or processes with default settings
                                     share a device; a process that owns its device may ask for more (160 of 256 measured best on an MI355X),
                                     N processes on one device for at most (compute units) / N each. */
    int32_t place_tries;          /* 0 / 1 = off.  T > 1: gie_create times the Mark + commit sweep's memory pattern on the mapper's four large
                                     planes and re-allocates each up to T - 1 times, keeping the faster physical placement (the same kernel runs
                                     0.76 or 0.84 ms from one allocation to the next on an MI355X).  Costs tens of milliseconds and, transiently,
                                     a second copy of one plane; only for volumes of 16 M voxels and more.  Off by default: create is then
                                     deterministic and holds no more memory than the mapper keeps. */
    int32_t reserved[3];
} gie_config;

/* MulScanParam, include/cuda_toolkit/occupancy/vlp16/multiscan_param.h:4-27 */
typedef struct gie_multiscan_param {
    int32_t scan_num, ring_num;
    float max_r, theta_inc, theta_min, phi_inc, phi_min;
} gie_multiscan_param;

/* CamParam, include/cuda_toolkit/occupancy/realsense/camera_param.h:4-27 */
typedef struct gie_cam_param {
    int32_t rows, cols;
    float cx, cy, fx, fy;
    int32_t valid_nan;
} gie_cam_param;

/* ScanParam, include/cuda_toolkit/occupancy/hokuyo/scan_param.h:4-19 */
typedef struct gie_scan_param {
    int32_t scan_num;
    float max_r, theta_inc, theta_min;
} gie_scan_param;

/* One global voxel as planners see it (GlbVoxel, voxmap_utils.cuh:29-44). */
typedef struct gie_voxel {
    uint8_t occ_val;
    int8_t vox_type;
    int16_t pad;
    int32_t dist_sq;
    int32_t coc[3];
} gie_voxel;

/* CostMap.msg header fields (msg/CostMap.msg:1-15, volumetric_mapper.cpp:375-389). */
typedef struct gie_costmap_hdr {
    int32_t x_size, y_size, z_size;
    float x_origin, y_origin, z_origin;
    float width;
    uint8_t type; /* TYPE_EDT = 1; TYPE_NF1 = 2 from gie_read_costmap_nf1 */
    uint8_t pad[3];
} gie_costmap_hdr;

/* SeenDist payload element, local_batch.h:19-24 (8 bytes: float d; bool s; bool o; 2 bytes of tail padding).
 * d = _edt_D in VOXEL units; o = `bool` converted from the voxel's type (local_batch.h:389): 1 for FREE /
 * OCCUPIED / FNT, 0 for UNKNOWN; s is never written by the reference (here: 0, padding 0). */
typedef struct gie_seendist {
    float d;
    uint8_t s;
    uint8_t o;
    uint8_t pad[2];
} gie_seendist;

/* Per-frame counters (the reference prints/keeps: glb_hash_map.cu:86,170-172; wave_helper.h). */
typedef struct gie_frame_stats {
    int32_t frame;            /* map_ct (_time)                                  */
    int32_t blocks_total;     /* blocks in the pool                              */
    int32_t blocks_new;       /* "New blocks allocated"                          */
    int32_t seeds_a, seeds_b, seeds_c; /* after obtainFrontiers                 */
    int32_t front_b, front_c; /* |B| after wave A, |C| after wave B              */
    int32_t visits_a, visits_b, visits_c; /* frontier entries expanded          */
    int32_t levels_a, levels_b, levels_c;
    float us_ogm, us_fuse, us_edt, us_merge; /* device time of the last step's stages; filled while gie_profile_enable is on, else 0 */
    int64_t total_visits_a, total_visits_b, total_visits_c; /* since gie_create */
    int32_t known_tiles;      /* 8x8x8 tiles of the local volume that hold a known voxel (what Mark / commit sweep) */
    int32_t frontier_tiles;   /* tiles obtainFrontiers looks at voxel by voxel (the voxels on the six faces come on top) */
} gie_frame_stats;

const char *gie_last_error(void);

/* LocMap::LocMap + create_gpu_map (local_batch.h:35-89), GlbHashMap::GlbHashMap
 * (glb_hash_map.cu:9-47), setupRotationPlan (volumetric_mapper.cpp:344-373), warmupCuda. */
gie_mapper *gie_create(const gie_config *cfg);
void gie_destroy(gie_mapper *h);

/* odom2trans/trans2proj (projection.h:14-33) + LocMap::calculate_pivot_origin /
 * calculate_update_pivot (local_batch.h:129-166).  Also advances the map tick (_time++).
 * Limits (GIE_ERR_INVALID beyond them; a refused pose changes nothing: no tick, no pivot):
 *  position   every component finite with |pos_k| <= 1.0e6 m, AND its voxel gie_pos2coord(pos_k) = floor(pos_k / w + 0.5) within
 *             +-900000: at w = 0.125 m that is +-112.5 km; above w = 10/9 m the limit in metres is the nearer one.  Both ends are
 *             accepted.  Out there one float32 ulp of a world coordinate is 1/128 m (>= 65536 m): poses, sensor points and query
 *             points are rounded to that before the library sees them, and results are bit for bit the oracle's all the same.
 *  900000     the reference calls a closest obstacle with a coordinate ABOVE 900000 invalid (invalid_coc_glb,
 *             voxmap_utils.cuh:167-172; its "no obstacle" key is 999999) and so does this library: stored records of voxels
 *             outside the local volume whose obstacle lies above +900000 on an axis are never propagated by the waves.  The rule
 *             is one-sided (nothing happens at -900000), and it only matters for poses within half a volume of +900000, where a
 *             map differs from the same drive elsewhere in such records.
 *  tick       the 18 low bits of the tick stamp the wave planes; at every multiple of 2^18 updates (7.3 h at 10 Hz) gie_set_pose
 *             clears the stamps once.  Nothing observable changes there: maps and statistics go on as the oracle's do, and
 *             gie_frame_stats.frame keeps counting. */
int gie_set_pose(gie_mapper *h, const float pos[3], const float quat_wxyz[4]);

/* PntcldMapMaker::updateLocalOGM (pntcld_map_maker.cpp:63-73) →
 * PNTCLD_RAYCAST::localOGMKernels (pntcld_raycast.cu:105-117). xyz: n sensor-frame points.
 * n == 0 is a valid (empty) scan.  A point whose global-frame coordinates are not finite or lie
 * beyond +-1e6 m is ignored (gie_math.h gie_point_ok; undefined in the reference). */
int gie_ogm_pointcloud(gie_mapper *h, const float *xyz, int n);
int gie_ogm_pointcloud_dev(gie_mapper *h, const float *d_xyz, int n);
/* Vlp16MapMaker::updateLocalOGM (vlp16_map_maker.cpp:51-71) → VLP_FAST::localOGMKernels
 * (vlp16_fast.cu:89-97). ranges: ring-major [ring_num][scan_num] horizontal ranges. */
int gie_ogm_multiscan(gie_mapper *h, const float *ranges, const gie_multiscan_param *p);
int gie_ogm_multiscan_dev(gie_mapper *h, const float *d_ranges, const gie_multiscan_param *p);
/* RealsenseMapMaker::updateLocalOGM (realsense_map_maker.cpp:46-52) →
 * REALSENSE_FAST::localOGMKernels (realsense_fast.cu:97-104). depth: row-major rows x cols. */
int gie_ogm_depth(gie_mapper *h, const float *depth, const gie_cam_param *p);
int gie_ogm_depth_dev(gie_mapper *h, const float *d_depth, const gie_cam_param *p);
/* HokuyoMapMaker::updateLocalOGM (hokuyo_map_maker.cpp:44-50) → HOKUYO_FAST::localOGMKernels. */
int gie_ogm_scan2d(gie_mapper *h, const float *ranges, const gie_scan_param *p);
/* A scan that arrives already classified: labels[idx] for every voxel of the local volume
 * (x fastest), GIE_VOX_UNKNOWN = not observed, GIE_VOX_FREE, GIE_VOX_OCCUPIED (anything else is
 * ignored).  This is the state the reference's projective kernels leave behind — `_inst_type` plus
 * the block key of every observed voxel (setLocalOccupancy: vlp16_fast.cu:76-86,
 * realsense_fast.cu:80-93, hokuyo_fast.cu:68-80) — without a sensor model in front of it; fused
 * like any projective scan (updateHashOGMWithSensor).  It is how the sensor-less synthetic world
 * of BASELINE config 5 (occupancy from a hash of the voxel, full observation) is
 * fed.  The robot sphere of for_motion_planner is forced FREE as in every OGM kernel. */
int gie_ogm_labels(gie_mapper *h, const int8_t *labels);
/* _dev: a device-resident plane, copied into the mapper's own scan plane by this call's kernel on the mapper's stream
 * (gie_get_stream): d_labels may be reused once that kernel has run, as with every other gie_ogm_*_dev entry point. */
int gie_ogm_labels_dev(gie_mapper *h, const int8_t *d_labels);
/* _dev_borrow (round 6; rounds 5's gie_ogm_labels_dev did this unasked): the plane MAY be read IN PLACE by gie_fuse instead (no copy
 * into `_inst_type`, no reset of it: 2 bytes per voxel less) — when the volume's X is a multiple of 16, d_labels is 16-byte aligned and
 * for_motion_planner is off; *borrowed (may be NULL) says whether it is.  The call itself then launches nothing: gie_fuse reads the
 * labels, its block allocation included (only where a block is missing).  A borrowed plane must stay unchanged until the gie_fuse /
 * gie_step of this map update has been executed on the mapper's stream — or until another gie_ogm_* / gie_read_ogm call, which
 * copies it first. */
int gie_ogm_labels_dev_borrow(gie_mapper *h, const int8_t *d_labels, int *borrowed);

/* Ext_Obs_Wrapper boxes as consumed by the fuse kernels (pre_map.cu:80-101,
 * unify_helper.cuh:68-86). ll/ur: n x 3 floats (metres); active: n flags. Box 0 is the inverted
 * "fence". n = 0 clears. */
int gie_set_ext_boxes(gie_mapper *h, const float *ll, const float *ur, const uint8_t *active, int n);

/* GlbHashMap::updateHashOGM (glb_hash_map.cu:115-143): allocHashTB + updateHashOGMWith*.  Needs a scan: GIE_ERR_INVALID when no
 * gie_ogm_* call has been made since the last gie_fuse (an update that only changes the external boxes feeds an empty scan:
 * gie_ogm_pointcloud(h, NULL, 0)). */
int gie_fuse(gie_mapper *h);
/* EDT_OCC::batchEDTUpdate (local_edt.cu:7-28). */
int gie_batch_edt(gie_mapper *h);
/* GlbHashMap::mergeNewObsv (glb_hash_map.cu:146-207).  One merge per map update: GIE_ERR_INVALID without a gie_fuse since the
 * last merge (the seed counters and barrier words of the wavefront kernel are cleared with the frame). */
int gie_merge(gie_mapper *h);
/* The two halves of gie_merge for a TILED run (gie_set_tile): gie_merge_begin_tiled = MarkLimitedObserve + commit of the
 * Mark-time pairs, so that the face layers exported next are THIS map update's state; gie_merge_end = obtainFrontiers +
 * waves + commit, run after the neighbours' layers have been imported.  gie_merge = begin + end. */
int gie_merge_begin(gie_mapper *h);
int gie_merge_begin_tiled(gie_mapper *h);
int gie_merge_end(gie_mapper *h);
/* fuse + batch_edt + merge, asynchronous on the mapper's stream. */
int gie_step(gie_mapper *h);
/* GPU_DEV_SYNC (cuda_macro.h:38); also surfaces device-side capacity errors. */
int gie_sync(gie_mapper *h);

/* LocMap::copy_edt_2_host / copy_ogm_2_host (local_batch.h:370-378) + the pair contents.
 * Any pointer may be NULL. edt: N floats (_edt_D, voxel units); type: N (_glb_type);
 * dist_sq: N (pair distance); coc_xyz: 3N global coords of the closest obstacle
 * (GIE_EMPTY_VALUE x3 when there is none). */
int gie_read_local(gie_mapper *h, float *edt, int8_t *type, int32_t *dist_sq, int32_t *coc_xyz);
/* Intermediate state for parity tests: OGM scan labels / hit-miss counters (before fuse).  After a
 * ray-cast scan the FREE / OCCUPIED labels of the counted cells (getAllocKeys) are only written
 * when this call asks for them: fuse works from the counters. */
int gie_read_ogm(gie_mapper *h, int8_t *inst_type, int32_t *ray_count);
/* Batch EDT result before the merge: dist² (_aux) and local closest-obstacle coords
 * (_coc_idx_aux unpacked; -1 x3 when the volume holds no obstacle).  The map update itself only
 * produces this plane where it is read (voxels of tiles that hold a known voxel); this call
 * completes it over the whole volume first. */
int gie_read_batch_edt(gie_mapper *h, int32_t *dist_sq, int32_t *coc_xyz_local);
/* LocMap::convertCostMap (local_batch.h:382-391) + setupEDTmsg4Motion
 * (volumetric_mapper.cpp:375-389). payload: N gie_seendist. */
int gie_read_costmap(gie_mapper *h, gie_seendist *payload, gie_costmap_hdr *hdr);
/* The same payload for consumers that cannot afford the stall (at 512^3 it is 1.07 GB per frame; the reference's blocking copy into
 * pageable memory, local_batch.h:370-391, was written for volumes 100x smaller):
 *  gie_read_costmap_dev   into a DEVICE buffer of the caller's (a GPU planner), asynchronous on the mapper's stream;
 *  gie_costmap_publish    conversion on the mapper's stream + ONE asynchronous copy into pinned host memory the library owns, on a
 *                         copy stream of its own: returns at once, and the next map update does not queue up behind the copy;
 *  gie_costmap_acquire    waits for the last publish and hands out its payload (N gie_seendist in pinned memory; valid until the
 *                         publish after the next one — two buffers alternate). */
int gie_read_costmap_dev(gie_mapper *h, gie_seendist *d_payload, gie_costmap_hdr *hdr);
int gie_costmap_publish(gie_mapper *h, gie_costmap_hdr *hdr);
int gie_costmap_acquire(gie_mapper *h, const gie_seendist **payload);
/* Hash lookup + retrive_vox_D (voxmap_utils.cuh:94-132) for n global coords. Voxels of
 * unallocated blocks come back as a default GlbVoxel (UNKNOWN, EMPTY_VALUE, EMPTY_KEY). */
int gie_query_global(gie_mapper *h, const int32_t *xyz, int n, gie_voxel *out);
/* Device-side access to the global map for GPU planners — the integration the reference recommends (README.md:163-165:
 * get_VB_key / get_voxID_in_VB / hash_table_D lookups inside the planner's own kernels, voxmap_utils.cuh:94-132): d_xyz (n x 3)
 * and d_out (n) are DEVICE buffers, the lookup kernel is enqueued on the mapper's stream (gie_get_stream), nothing is copied and
 * the host does not wait.  Same records as gie_query_global. */
int gie_query_global_dev(gie_mapper *h, const int32_t *d_xyz, int n, gie_voxel *d_out);
int gie_get_stats(gie_mapper *h, gie_frame_stats *out);

/* ---- signed distance field of the local volume and interpolated distance / gradient queries, for gradient-based planners
 * (the reference lists "Signed distance" as a feature in development, README.md "Additional features").  No counterpart in the
 * reference's code.
 *
 * The field covers the local volume only, in the current frame: it is what gie_read_local / gie_read_costmap would read at the
 * same point in the mapper's stream.
 *  occupied(v)        glb_type[v] == GIE_VOX_OCCUPIED.  UNKNOWN, FREE and FNT count as non-occupied, as for the positive EDT.
 *  inside_dist_sq(v)  0 when v is not occupied; otherwise the exact squared Euclidean distance, in voxels and as an integer, from v
 *                     to the nearest non-occupied voxel OF THE LOCAL VOLUME; -1 when the volume holds no non-occupied voxel.
 *  sdf(v)             voxel units, like _edt_D and gie_seendist.d:
 *                       inside_dist_sq(v) <= 1:  sdf(v) = the `edt` gie_read_local returns for v, bit for bit;
 *                       inside_dist_sq(v) >  1:  sdf(v) = 1.0f - sqrtf((float)inside_dist_sq(v));
 *                       inside_dist_sq(v) == -1: sdf(v) = -(float)max_loc_dist_sq (X² + Y² + Z²), the mirror of the positive
 *                                                side's value for "no obstacle".
 *                     The usual "positive minus negative plus one voxel" convention: the surface layer of an obstacle stays at
 *                     0, deeper voxels go negative.  The field differs from the EDT ONLY at occupied voxels without a
 *                     non-occupied face neighbour in the volume.
 * Query at a point p (metres, world frame: the frame of gie_set_pose):
 *  u_k = p_k / w - (float)pvt_k    continuous local coordinate (voxel centres at integers: gie_pos2coord = floor(p/w + 0.5));
 *  axis with size_k >= 2:          inside iff 0 <= u_k <= size_k - 1; i0 = min(floor(u_k), size_k - 2), t = u_k - i0;
 *  axis with size_k == 1:          inside iff -0.5 <= u_k < 0.5; the field is constant along it, its gradient component is 0;
 *  dist    trilinear interpolation of sdf over the 8 corners, times w: metres;
 *  grad    the analytic gradient of that interpolant (n x 3, x y z per point): m/m;
 *  flags   bit 0 inside the volume, bit 1 all corners known (type != UNKNOWN), bit 2 some corner occupied;
 *  outside the volume: dist = NaN, grad = 0, flags = 0.
 * Cache: inside_dist_sq is computed on the device at the first of these calls after anything that can change a committed type
 * (every gie_fuse / gie_step and the frontier pass of gie_merge) and kept until the next such change.  A mapper that never calls
 * them allocates nothing and launches nothing; the first call allocates 4 bytes per voxel plus two bit planes whose rows are
 * padded to 64-bit words (16 * ceil(X/64) / X bytes per voxel: 4.25 bytes per voxel in all when X is a multiple of 64, at most
 * 5 when X >= 22), freed by gie_destroy.  Nothing of the map update reads them.
 * Arguments: sdf / inside_dist_sq are N values each (x fastest), either may be NULL; dist (n), grad (3n) and flags (n) may each be
 * NULL, but not all three; n == 0 is valid; a bad argument gives GIE_ERR_INVALID.  The host forms synchronise; the _dev forms take
 * DEVICE buffers and are enqueued on the mapper's stream (gie_get_stream) like gie_query_global_dev: nothing is copied, the host
 * does not wait.
 * A tiled mapper (gie_set_tile with a non-zero offset, or whole != local_size) gets GIE_ERR_INVALID from all four: its inside
 * distances would stop at the tile's faces.
 * gie_profile_read: "sdf" = the inside distances and the gie_read_sdf* exports, "sdf_query" = the queries (the last two entries). */
int gie_read_sdf(gie_mapper *h, float *sdf, int32_t *inside_dist_sq);
int gie_read_sdf_dev(gie_mapper *h, float *d_sdf, int32_t *d_inside_dist_sq);
int gie_query_sdf(gie_mapper *h, const float *xyz, int n, float *dist, float *grad, uint8_t *flags);
int gie_query_sdf_dev(gie_mapper *h, const float *d_xyz, int n, float *d_dist, float *d_grad, uint8_t *d_flags);

/* ---- NF1 navigation function of the local volume, for gradient planners and frontier exploration (msg/CostMap.msg reserves
 * TYPE_NF1 = 2 for it; the reference never writes it).  No counterpart in the reference's code.
 *
 * Everything is over the local volume at the point of the mapper's stream where gie_nf1_compute* is enqueued; type(v) and edt(v)
 * are exactly what gie_read_local would return there (edt in voxel units, as gie_seendist.d).
 *  traversable(v)  type(v) is FREE or FNT (or UNKNOWN, with GIE_NF1_UNKNOWN_TRAVERSABLE) and edt(v) >= clearance (a float
 *                  comparison; clearance in voxel units, finite and >= 0, otherwise GIE_ERR_INVALID).
 *  sources         traversable voxels among: the voxel of each goal point g (metres, world frame) at gie_pos2coord(g_k, w) - pvt_k,
 *                  points outside the volume (or not finite) ignored; every FNT voxel, with GIE_NF1_FROM_FRONTIERS (the distance
 *                  to the nearest reachable frontier, the exploration guide).
 *  nf1(v)          int32: for a traversable voxel with a path to a source, the number of steps of the shortest 6-connected path
 *                  from v to a source whose every voxel is traversable and inside the volume (sources 0); -1 everywhere else.
 * The field is kept until the next compute and refers to the pivot gie_get_pivot returned when it was enqueued; map updates do not
 * change it.  n_sources: the number of sources (host int32 / device int32 of the caller's; either may be NULL).  n == 0 is valid.
 * Path: one descent per start point s (mapped like the goals, at the field's pivot): len = 0 when s is outside the volume or
 *  nf1(s) < 0; otherwise s = v0 .. vk, k = nf1(s), v_{i+1} = the first 6-neighbour of v_i in the order -x +x -y +y -z +z whose
 *  value is nf1(v_i) - 1.  path_xyz: max_len points (3 int32 each, GLOBAL voxel coordinates = local + pivot) per start;
 *  len[i] = k + 1 even when that exceeds max_len (only max_len points are written: truncated iff len > max_len).
 * CostMap (TYPE_NF1): hdr as gie_read_costmap with type = 2 and the origin of the field's pivot; payload d = (float)nf1(v), or
 *  -1.0f where nf1(v) = -1; o = type(v) != UNKNOWN at compute time (as gie_read_costmap's o); s = 0.
 * The host forms synchronise; the _dev forms take DEVICE buffers and are enqueued on the mapper's stream without a host wait (the
 * whole propagation is one persistent launch of gie_config.wave_workgroups workgroups, a grid barrier per BFS level: a few
 * microseconds per level, so a winding field of many thousand levels holds those compute units for as many times that).
 * Like the wavefront launches, that launch joins the device's chain of grid-barrier launches: while more than one mapper lives on
 * a device, it starts after every such launch enqueued before it by any mapper and before any enqueued after it, so it is never
 * resident half and half with another mapper's map update (which then waits for it).
 * If a grid barrier of that launch times out (its workgroups were kept off the device by another process), the next sync reports
 * GIE_ERR_TIMEOUT through the error word the map update uses, with its own message; the field is then incomplete (some values -1
 * or too large) until the next compute; a descent stops early on it.  The map itself is not affected.
 * gie_read_nf1*, gie_nf1_path* and gie_read_costmap_nf1* return GIE_ERR_INVALID before the first compute; a tiled mapper gets
 * GIE_ERR_INVALID from all of them.
 * Memory: allocated at the first compute (gie_dalloc, freed by gie_destroy): 4 bytes per voxel for the field, five bit planes with
 * rows padded to 64-bit words (40 * ceil(X/64) / X bytes per voxel: 0.625 when X is a multiple of 64), 12 bytes per tile of
 * 64 x 8 x 8 voxels: 4.63 bytes per voxel in all when X is a multiple of 64.  Nothing of the map update reads them. */
#define GIE_NF1_UNKNOWN_TRAVERSABLE 1
#define GIE_NF1_FROM_FRONTIERS 2
typedef struct gie_nf1_param {
    float clearance;        /* voxel units */
    int32_t flags;          /* GIE_NF1_* */
    int32_t reserved[2];    /* 0 */
} gie_nf1_param;
int gie_nf1_compute(gie_mapper *h, const float *goal_xyz, int n, const gie_nf1_param *p, int32_t *n_sources);
int gie_nf1_compute_dev(gie_mapper *h, const float *d_goal_xyz, int n, const gie_nf1_param *p, int32_t *d_n_sources);
int gie_read_nf1(gie_mapper *h, int32_t *nf1);
int gie_read_nf1_dev(gie_mapper *h, int32_t *d_nf1);
int gie_nf1_path(gie_mapper *h, const float *start_xyz, int n, int max_len, int32_t *path_xyz, int32_t *len);
int gie_nf1_path_dev(gie_mapper *h, const float *d_start_xyz, int n, int max_len, int32_t *d_path_xyz, int32_t *d_len);
int gie_read_costmap_nf1(gie_mapper *h, gie_seendist *payload, gie_costmap_hdr *hdr);
int gie_read_costmap_nf1_dev(gie_mapper *h, gie_seendist *d_payload, gie_costmap_hdr *hdr);

/* ---- frontier clusters: the connected components of the local volume's FNT voxels, filtered by size, each with a goal a planner
 * can drive to.  The reference's README says of its frontiers ("Frontiers for exploration"): "You may need to do some post-process
 * to filter out the noise." — this is that post-process, on the device.  No counterpart in the reference's code.
 *
 * Everything is over the local volume at the point of the mapper's stream where gie_frontier_compute* is enqueued; type(v) and
 * edt(v) are exactly what gie_read_local would return there.  id(v) = (z * Y + y) * X + x is the local linear index.
 *  member(v)     type(v) == GIE_VOX_FNT and edt(v) >= clearance (a float comparison; clearance in voxel units, finite and >= 0,
 *                otherwise GIE_ERR_INVALID: the rule of NF1's traversable, so with equal clearance every member is a legal NF1 source).
 *  adjacent      two members that differ by at most 1 on every axis and are not equal (connectivity = 26), or that are face
 *                neighbours (connectivity = 6).  Any other value: GIE_ERR_INVALID.  Frontier sheets are staircase surfaces: 26
 *                is what callers normally want, 6 is the strict form.
 *  component     a class of the transitive closure of `adjacent` inside the volume.  Its label is the smallest id of its members,
 *                its size the number of members.  Both are independent of any schedule.
 *  kept          size >= min_size (min_size >= 1, otherwise GIE_ERR_INVALID): the noise filter.
 *  label plane   int32 per voxel (x fastest): -1 not a member; -2 member of a component that is not kept; otherwise the label.
 *  cluster record  one gie_frontier_cluster per kept component, in ascending order of label.
 *                centroid_k = ((float)((double)sum_k / (double)size) + (float)pvt_k) * w, in this order of operations.
 *                rep: with c_k = (2 * sum_k + size) / (2 * size) (integer division: the centroid rounded half up to a voxel), the
 *                member that minimises |v - c|^2 (integers), ties to the smaller id.  The centroid of a curved sheet is usually not
 *                a frontier voxel and may lie inside an obstacle; rep always is a member, so with equal clearance it is a legal
 *                NF1 goal.
 *  capacity      max_clusters >= 0 (otherwise GIE_ERR_INVALID).  n_clusters is the number of KEPT components even when it exceeds
 *                max_clusters; only the first max_clusters records (ascending label) are produced (the convention of
 *                gie_nf1_path's len > max_len).  n_voxels = members in kept components.  The label plane is complete whatever
 *                the capacity.  d_counts (device, 2 int32, may be NULL) = { n_clusters, n_voxels }.
 *  readers       gie_read_frontier_clusters*: out and goal_xyz hold max_clusters (of the compute) entries, either may be NULL.
 *                out: the records produced; entries beyond them are left as they are.  goal_xyz (3 floats per entry):
 *                (float)rep_k * w for the records produced, NaN for the rest — so the whole array can be handed to
 *                gie_nf1_compute_dev(h, d_goal_xyz, max_clusters, ...) without the host ever learning the count (NF1 ignores
 *                goals that are not finite).  gie_pos2coord((float)rep_k * w, w) = floorf(p / w + 0.5f) gives rep_k back while
 *                |rep_k| < 2^20: product and quotient are each off by at most a few ulp of a value below 2^20 (3 * 2^-4 of a
 *                voxel in all), inside the half-voxel margin.  *n_clusters as the compute's.
 * The result is kept until the next compute and refers to the pivot gie_get_pivot returned when the compute was enqueued (as NF1);
 * map updates do not change it.  The readers return GIE_ERR_INVALID before the first compute; a NULL param and a tiled mapper
 * (its components would stop at the tile's faces) get GIE_ERR_INVALID from all six.
 * The host forms synchronise; the _dev forms take DEVICE buffers and are enqueued on the mapper's stream without a host wait.  A
 * compute is a fixed sequence of launches (about a dozen, whatever the data), none with a grid barrier.
 * Memory: allocated at the first compute (gie_dalloc, freed by gie_destroy): 8 bytes per voxel (the union-find forest and the
 * sizes), two bit planes with rows padded to 64-bit words and 8 bytes per such word (0.375 bytes per voxel when X is a multiple of
 * 64), and 80 bytes per record of the largest max_clusters asked for.  Nothing of the map update reads them. */
typedef struct gie_frontier_cluster {   /* 80 bytes */
    int32_t label;          /* smallest local linear index of a member */
    int32_t size;
    int32_t lo[3], hi[3];   /* bounding box, GLOBAL voxel coordinates (local + pivot), both inclusive */
    int32_t rep[3];         /* representative member, GLOBAL voxel coordinates */
    float centroid[3];      /* metres, world frame */
    int64_t sum[3];         /* sums of the members' LOCAL coordinates */
} gie_frontier_cluster;
typedef struct gie_frontier_param {
    float clearance;        /* voxel units */
    int32_t min_size;
    int32_t connectivity;   /* 6 or 26 */
    int32_t max_clusters;
    int32_t reserved[2];    /* 0 */
} gie_frontier_param;
int gie_frontier_compute(gie_mapper *h, const gie_frontier_param *p, int32_t *n_clusters, int32_t *n_voxels);
int gie_frontier_compute_dev(gie_mapper *h, const gie_frontier_param *p, int32_t *d_counts);
int gie_read_frontier_clusters(gie_mapper *h, gie_frontier_cluster *out, float *goal_xyz, int32_t *n_clusters);
int gie_read_frontier_clusters_dev(gie_mapper *h, gie_frontier_cluster *d_out, float *d_goal_xyz, int32_t *d_n_clusters);
int gie_read_frontier_labels(gie_mapper *h, int32_t *labels);
int gie_read_frontier_labels_dev(gie_mapper *h, int32_t *d_labels);

/* ---- line of sight: is the straight segment between two points clear, and how much would a sensor see from a pose?  The two
 * questions between "clusters with goals" and "drive there": shortcutting gie_nf1_path's staircase, the collision test of a sampling
 * planner, the information-gain half of frontier exploration.  The reference's README: "To access the global EDT directly, you are
 * recommended to implement a GPU-based motion planner together with GIE-mapping."  No counterpart in the reference's code.
 *
 * Everything is over the local volume at the point of the mapper's stream where gie_los_prepare* is enqueued; type(v) and edt(v) are
 * exactly what gie_read_local would return there.  Every later call refers to that prepare and its pivot until the next prepare;
 * map updates do not change a result (as NF1 and the clusters).
 *  opaque(v)     type(v) == GIE_VOX_OCCUPIED, or type(v) == GIE_VOX_UNKNOWN with GIE_LOS_UNKNOWN_OPAQUE, or clearance > 0 and
 *                edt(v) < clearance (a float comparison; clearance in voxel units, finite and >= 0, otherwise GIE_ERR_INVALID:
 *                NF1's rule).  With clearance == 0 edt(v) has no part in it.  Flags other than GIE_LOS_UNKNOWN_OPAQUE:
 *                GIE_ERR_INVALID.  n_opaque = the number of opaque voxels (host int32 / device int32 of the caller's, may be NULL).
 *  voxel line    L(a, b), for local voxels a and b: the voxels whose cube shares a piece of POSITIVE length with the straight
 *                segment between the two voxel centres, in the order of those pieces from a to b.  L(a, a) = (a).  The walk: with
 *                n_k = |b_k - a_k|, crossing j (1..n_k) of axis k lies at t = (2j - 1) / (2 n_k); take the smallest pending t and
 *                step ALL axes tied at it together, until none is pending.  A line through an edge or a corner of the grid makes
 *                a diagonal move: the voxels that touch it only there are not on it.  (2 j_a - 1) * n_b against (2 j_b - 1) * n_a
 *                decides the order of two crossings, exactly in 32-bit integers (gie_create keeps every side <= 1024).
 *                L(b, a) is L(a, b) reversed; no voxel repeats; 1 + max n_k <= len <= 1 + n_x + n_y + n_z.
 *  segment       a pair of points (metres, world frame), each mapped like NF1's goals: gie_pos2coord(p_k, w) - pvt_k.  Result,
 *                one gie_los_hit per segment:
 *                  first    index along L(a, b) of the first opaque voxel (a has index 0); -1 when none is opaque; -2 when an
 *                           endpoint is not finite or lies outside the volume (every other field is then 0);
 *                  len      the number of voxels of L(a, b);
 *                  hit      the first opaque voxel, GLOBAL coordinates (local + pivot); b's when first == -1;
 *                  min_edt  the minimum of edt(v) over the voxels of index 0 .. first (all of the line when first == -1): the
 *                           exact float minimum of the values at prepare time, voxel units.
 *  view gain     per gie_view, with p = the voxel of pos (mapped like a segment's endpoint), d = v - p, rmin = r_min / w and
 *                rmax = r_max / w (float), voxel v is a CANDIDATE iff
 *                  v is inside the volume and v != p;
 *                  (float)|d|^2 >= rmin * rmin and (float)|d|^2 <= rmax * rmax (|d|^2 is an exact integer below 2^24: one
 *                  float product and one comparison on each side);
 *                  tan2_elev < 0, or (float)(d_z^2) <= tan2_elev * (float)(d_x^2 + d_y^2): the vertical band of a spinning lidar;
 *                  normal[i] . d >= 0 (an exact 64-bit integer dot product) for each i < n_planes: four planes make a camera's
 *                  frustum.
 *                A candidate is VISIBLE iff no voxel of L(p, v) other than v itself is opaque; p's own opacity is ignored, v may
 *                be anything.  gie_view_score: unknown / frontier / occupied = the visible candidates of type UNKNOWN / FNT /
 *                OCCUPIED, candidates = all candidates; all four are -1 when pos is not finite or lies outside the volume.  The
 *                counts are sums: they depend on no schedule.
 *                Refused with GIE_ERR_INVALID: r_min or r_max not finite, r_min < 0, r_min > r_max, tan2_elev NaN; in the host
 *                form also a view with n_planes outside 0..4 or a component of one of its n_planes normals beyond +-32767.  The
 *                _dev form never reads the views on the host: such a view scores -1 in all four fields there.
 * Arguments follow the NF1 section: n == 0 is valid; a NULL param, a NULL buffer that would be read or written, n < 0:
 * GIE_ERR_INVALID.  Everything but gie_los_prepare* returns GIE_ERR_INVALID before the first prepare.  A tiled mapper gets
 * GIE_ERR_INVALID from all ten: its lines would stop at the tile's faces.  The host forms synchronise (gie_los_prepare also when
 * n_opaque is NULL); the _dev forms take DEVICE buffers and are enqueued on the mapper's stream without a host wait.  Every call
 * is a fixed sequence of launches, none with a grid barrier.
 * gie_read_los_opaque*: N bytes of 0 / 1, x fastest.
 * Memory: allocated at the first prepare (gie_dalloc, freed by gie_destroy): the opaque bit plane with rows padded to 64-bit words
 * (8 * ceil(X/64) / X bytes per voxel: 0.125 when X is a multiple of 64), the types (1 byte per voxel) and edt (4 bytes per voxel)
 * of the prepare — a segment's min_edt and a view's counts have to be those of the prepare whatever the map does afterwards, so
 * they are copies.  Nothing of the map update reads them; a mapper that never calls gie_los_prepare* allocates and launches nothing.
 * gie_profile_read: "los" = prepare and the plane's reader, "los_query" = segments and gain (the two entries before "sdf"). */
#define GIE_LOS_UNKNOWN_OPAQUE 1
typedef struct gie_los_param {
    float clearance;        /* voxel units */
    int32_t flags;          /* GIE_LOS_* */
    int32_t reserved[2];    /* 0 */
} gie_los_param;
typedef struct gie_los_hit {            /* 24 bytes */
    int32_t first;
    int32_t len;
    int32_t hit[3];
    float min_edt;
} gie_los_hit;
typedef struct gie_view {               /* 64 bytes */
    float pos[3];           /* metres, world frame */
    int32_t n_planes;       /* 0..4 */
    int32_t normal[4][3];   /* inward normals of the half spaces, integers of magnitude <= 32767 */
} gie_view;
typedef struct gie_view_param {
    float r_min, r_max;     /* metres */
    float tan2_elev;        /* tan^2 of the half opening of the vertical band; < 0: no band */
    int32_t reserved;       /* 0 */
} gie_view_param;
typedef struct gie_view_score {         /* 16 bytes */
    int32_t unknown, frontier, occupied, candidates;
} gie_view_score;
int gie_los_prepare(gie_mapper *h, const gie_los_param *p, int32_t *n_opaque);
int gie_los_prepare_dev(gie_mapper *h, const gie_los_param *p, int32_t *d_n_opaque);
int gie_read_los_opaque(gie_mapper *h, uint8_t *opaque);
int gie_read_los_opaque_dev(gie_mapper *h, uint8_t *d_opaque);
int gie_los_segments(gie_mapper *h, const float *a_xyz, const float *b_xyz, int n, gie_los_hit *out);
int gie_los_segments_dev(gie_mapper *h, const float *d_a_xyz, const float *d_b_xyz, int n, gie_los_hit *d_out);
int gie_view_gain(gie_mapper *h, const gie_view *views, int n, const gie_view_param *vp, gie_view_score *out);
int gie_view_gain_dev(gie_mapper *h, const gie_view *d_views, int n, const gie_view_param *vp, gie_view_score *d_out);

/* ---- path shortcutting: any-angle waypoints from a polyline of voxels — what turns gie_nf1_path's 6-connected staircase into the
 * few straight legs a controller can follow: from the current waypoint, go to the farthest point of the path (within a look-ahead)
 * that is still visible over the opaque plane, repeat.  One call on the device, between gie_nf1_path_dev and whatever flies the
 * result.  No counterpart in the reference's code.
 *
 * Everything refers to the last gie_los_prepare* and its pivot (the line-of-sight section): its volume, its opaque plane, its edt
 * copy, its voxel line L(a, b).  Map updates do not change a result.
 *  input         the buffers of gie_nf1_path*: n paths of max_len points (3 int32 each, GLOBAL voxel coordinates), len[i] as that
 *                call left it: path i has m = min(max(len[i], 0), max_len) points v_0 .. v_{m-1}.  Any polyline of voxels is legal:
 *                it need not be 6-connected or come from NF1, points may repeat, lie outside the volume or be any int32 (local =
 *                global - pivot is computed in 64 bits).
 *  Clear(a, b)   a and b are inside the prepare's volume and no voxel of L(a, b), both ends included, is opaque.
 *  waypoints     indices k_0 = 0 < k_1 < .. < k_T = m - 1.  While k_t < m - 1, with K = lookahead:
 *                  J = { j : k_t < j <= min(k_t + K, m - 1) and Clear(v_{k_t}, v_j) };  k_{t+1} = max J,
 *                or, when J is empty, k_{t+1} = k_t + 1 and that leg is FORCED: the path stays connected and the caller learns that
 *                it is not valid there.  Visibility along a path is not monotone (a pillar's shadow hides a stretch of points and
 *                lets the ones behind it through): max J is the largest clear index of the whole window, not the last before the
 *                first blocked one.  count = T + 1; 0 when m = 0.
 *  gie_waypoint  record t: xyz = v_{k_t} as given, index = k_t.
 *                  t = 0: forced = 0; min_edt = edt(v_0) when v_0 is inside the volume, otherwise -1.0f.
 *                  a clear leg: forced = 0; min_edt = the exact float minimum of edt over all voxels of L(v_{k_{t-1}}, v_{k_t})
 *                  (values of the prepare, voxel units).
 *                  a forced leg: forced = 1; min_edt = -1.0f.
 *  gie_shortcut_info  count as above, even when it exceeds max_wp; forced = the number of forced legs; length = a float sum,
 *                started at 0.0f and accumulated in leg order t = 1 .. T: each CLEAR leg adds sqrtf((float)|v_{k_t} - v_{k_{t-1}}|^2)
 *                (an exact integer below 2^22: both ends lie inside a volume of sides <= 1024; sqrtf as in gie_read_sdf), a forced
 *                leg adds nothing.  Voxel units.
 *  capacity      wp holds max_wp records per path; only the first min(count, max_wp) of a path are written (the convention of
 *                gie_nf1_path's len > max_len), entries beyond them are left as they are.  info is complete whatever max_wp is.
 * GIE_ERR_INVALID: no prepare yet; a tiled mapper; a NULL param; lookahead outside 1..4096; max_wp < 0; n < 0; with n > 0,
 * max_len < 1 or a NULL path_xyz / len; wp NULL while max_wp > 0; wp and info both NULL.  n == 0 is valid and launches nothing.
 * The host form synchronises; it stages through the two scratch slots of the host forms and hands the entries of wp beyond a
 * path's records back as they were.  The _dev form takes DEVICE buffers and is enqueued on the mapper's stream without a host wait
 * or a read-back: one launch, no grid barrier, a wave per path (a leg costs its window's lines in chunks of 64 from the far end,
 * up to the first chunk with a clear one; a point outside the volume or in an opaque voxel costs nothing).
 * Memory: none is kept.  gie_profile_read: counted under "los_query". */
typedef struct gie_shortcut_param {     /* 16 bytes */
    int32_t lookahead;      /* K >= 1: a leg may reach at most K path points ahead; <= 4096 */
    int32_t max_wp;         /* >= 0: capacity of the waypoint array, per path */
    int32_t reserved[2];    /* 0 */
} gie_shortcut_param;
typedef struct gie_waypoint {           /* 24 bytes */
    int32_t xyz[3];         /* the path point, GLOBAL voxel coordinates, copied from the input */
    int32_t index;          /* its index in the input path */
    float   min_edt;        /* voxel units; -1.0f: a forced leg, or a first point outside the volume */
    int32_t forced;         /* 1: the leg that ends here is not a clear line */
} gie_waypoint;
typedef struct gie_shortcut_info {      /* 16 bytes, one per path */
    int32_t count;          /* waypoints of the path, even when > max_wp */
    int32_t forced;         /* forced legs */
    float   length;         /* voxel units */
    int32_t reserved;       /* 0 */
} gie_shortcut_info;
int gie_path_shortcut(gie_mapper *h, const int32_t *path_xyz, const int32_t *len, int n, int max_len,
                      const gie_shortcut_param *p, gie_waypoint *wp, gie_shortcut_info *info);
int gie_path_shortcut_dev(gie_mapper *h, const int32_t *d_path_xyz, const int32_t *d_len, int n, int max_len,
                          const gie_shortcut_param *p, gie_waypoint *d_wp, gie_shortcut_info *d_info);

/* ---- display clouds: the occupied voxels and the EDT slices a viewer shows, compacted on the device — the ROS-free half of
 * VOLMAPNODE::visualize (include/volumetric_mapper.h:181-357), which the reference runs every vis_interval map ticks over the local
 * volume and over every block of its CPU mirror.  Here the clouds come straight out of the local planes and the block pool: a caller
 * that only displays its map needs neither gie_read_local of the whole volume nor gie_stream_enable(1) and a mirror.
 *
 * A cloud is a set of gie_cloud_point records, one per SELECTED voxel; every value is exact and nothing depends on a schedule but
 * the order of the records.  w = voxel_width.
 *  local form    over the local volume at the point of the mapper's stream where the call is enqueued.  For local voxel v,
 *                g = v + pvt (gie_get_pivot); type(v) and edt(v) are exactly what gie_read_local would return there.
 *                  selected   iff bit type(v) of type_mask is set and z_lo <= g_z <= z_hi;
 *                  intensity  GIE_CLOUD_TYPE: (float)type(v);  GIE_CLOUD_DIST: edt(v) * w — one fp32 multiply; no voxel is dropped
 *                             for its distance, as in the reference's local loop.
 *                GIE_ERR_INVALID before the first gie_set_pose.
 *  global form   over every voxel g of every LIVE block of the pool: a block gie_query_global finds — its slot below the number
 *                handed out and its key not erased (gie_config.retain_radius_blocks).  Erased blocks and slots never handed out
 *                contribute nothing; an empty pool gives count 0.  With r = the record gie_query_global returns for g at that
 *                point of the stream (the records a fused update has left to the pair plane included; the call itself stores
 *                nothing: it does not write into the map at all):
 *                  selected   iff bit r.vox_type of type_mask is set, z_lo <= g_z <= z_hi and, with GIE_CLOUD_DIST,
 *                             0 <= r.dist_sq < 900000 (the reference's invalid_dist_glb, voxmap_utils.cuh:162-165: that literal,
 *                             not GIE_EMPTY_VALUE);
 *                  intensity  GIE_CLOUD_TYPE: (float)r.vox_type;  GIE_CLOUD_DIST: sqrtf((float)r.dist_sq) * w (sqrtf as in
 *                             gie_read_sdf).
 *  both          x, y, z = (float)g_k * w: coord2pos (local_batch.h:260-267), the convention of gie_read_frontier_clusters' goals.
 *                *count = the number of selected voxels, also when it exceeds max_points.  Exactly min(count, max_points) records
 *                are written: distinct selected voxels in unspecified order — which ones, when the cloud does not fit, is
 *                unspecified too (the convention of gie_stream_changed); entries beyond them are left as they were.
 *                max_points == 0 with a NULL out only counts.
 * GIE_ERR_INVALID: a NULL param; type_mask 0 or with bit 0 (UNKNOWN) or a bit >= 4 set; an intensity other than the two; z_lo > z_hi;
 * max_points < 0; non-zero reserved; a NULL out with max_points > 0; a NULL count together with a NULL out; a tiled mapper (its pool
 * holds ghost blocks of other tiles: all four refuse, as every planner section does); in the _dev forms a d_out that is not 16-byte
 * aligned.  Nothing is written then.
 * The host forms stage through the two scratch slots of the host forms and synchronise.  The _dev forms take DEVICE buffers and are
 * enqueued on the mapper's stream with no host wait and no read-back (the number of slots handed out is read on the device):
 * d_count is zeroed on the stream and accumulated in place; one memset and at most one launch, no grid barrier.  A call is legal
 * wherever gie_query_global is, also between gie_fuse and gie_merge of one update.  Map updates are not changed by it; a mapper
 * that never calls it allocates and launches nothing (a _dev call without d_count allocates one counter word).
 * Cost: GIE_CLOUD_TYPE reads 1 byte per voxel of the live blocks inside the band (a one-layer band: 64 bytes per block of that
 * block row, a key per block otherwise); GIE_CLOUD_DIST 8 bytes more per voxel that passed mask and band; 16 bytes per record.
 *
 * The reference's four clouds (volumetric_mapper.h:181-357; NOBAND = z_lo INT32_MIN, z_hi INT32_MAX):
 *   local OGM    gie_cloud_local   { 1 << GIE_VOX_OCCUPIED, GIE_CLOUD_TYPE, NOBAND }
 *   local EDT    gie_cloud_local   { 1 << GIE_VOX_FREE | 1 << GIE_VOX_OCCUPIED | 1 << GIE_VOX_FNT, GIE_CLOUD_DIST, NOBAND }
 *   global OGM   gie_cloud_global  { 1 << GIE_VOX_OCCUPIED, GIE_CLOUD_TYPE, NOBAND }   (its PointXYZ: ignore the intensity)
 *   global EDT   gie_cloud_global  { 1 << GIE_VOX_FREE | 1 << GIE_VOX_OCCUPIED | 1 << GIE_VOX_FNT, GIE_CLOUD_DIST,
 *                                    z_lo = z_hi = gie_pos2coord(vis_height, w) }
 * and { 1 << GIE_VOX_FNT, GIE_CLOUD_TYPE } is the frontier display.
 * gie_profile_read: "cloud" = all four, one bracket per call (the entry before "los"). */
#define GIE_CLOUD_TYPE 0            /* intensity = (float)vox_type                  */
#define GIE_CLOUD_DIST 1            /* intensity = the voxel's distance, metres     */
typedef struct gie_cloud_param {    /* 32 bytes */
    uint32_t type_mask;     /* bit t set: voxels of type t (GIE_VOX_FREE / OCCUPIED / FNT) are selected */
    int32_t  intensity;     /* GIE_CLOUD_TYPE or GIE_CLOUD_DIST */
    int32_t  z_lo, z_hi;    /* GLOBAL voxel z, both inclusive; INT32_MIN .. INT32_MAX = no band */
    int32_t  max_points;    /* >= 0: capacity of `out` */
    int32_t  reserved[3];   /* 0 */
} gie_cloud_param;
typedef struct gie_cloud_point { float x, y, z, intensity; } gie_cloud_point;   /* 16 bytes: PCL's PointXYZI without padding */
int gie_cloud_local(gie_mapper *h, const gie_cloud_param *p, gie_cloud_point *out, int32_t *count);
int gie_cloud_local_dev(gie_mapper *h, const gie_cloud_param *p, gie_cloud_point *d_out, int32_t *d_count);
int gie_cloud_global(gie_mapper *h, const gie_cloud_param *p, gie_cloud_point *out, int32_t *count);
int gie_cloud_global_dev(gie_mapper *h, const gie_cloud_param *p, gie_cloud_point *d_out, int32_t *d_count);

/* ---- global block summaries: one record per 8 x 8 x 8 block of everything mapped so far, for an exploration planner.  Every planner
 * section above answers questions about the local volume, which moves with the robot; a frontier the robot drove past stays in the
 * global map (g_type keeps GIE_VOX_FNT once the voxel has left the volume) and only gie_query_global (which must know where to
 * look), the display clouds (16 bytes per VOXEL) or the changed-block stream and a CPU mirror can see it.  This is gie_cloud_global's
 * definition at block resolution: a pure reduction over the block pool.  No counterpart in the reference's code.
 *
 * A block has the coordinate k = (global voxel >> 3) on every axis (arithmetic shift: voxel -1 lies in block -1).
 *  which voxels   every voxel g of every LIVE block of the pool, as in gie_cloud_global: the block's slot below the number handed
 *                 out and its key not erased (gie_config.retain_radius_blocks); an empty pool has none.  With r = the record
 *                 gie_query_global returns for g at the point of the mapper's stream where the call is enqueued (the records a
 *                 fused update has left to the pair plane included; the call stores nothing):
 *                   n_free, n_occupied, n_fnt   the number of the block's voxels with r.vox_type FREE, OCCUPIED, FNT (0..512 each;
 *                                               UNKNOWN = 512 - their sum);
 *                   fnt_voxel                   the least in-block index (g_x & 7) * 64 + (g_y & 7) * 8 + (g_z & 7) — the order of
 *                                               gie_stream_changed's blocks — of an FNT voxel, 0xffff when there is none;
 *                   free_voxel                  the same over the FREE and FNT voxels;
 *                   min_dist_sq                 with GIE_BLOCKS_DIST the least r.dist_sq over the block's FREE and FNT voxels with
 *                                               0 <= r.dist_sq < 900000 (the display clouds' validity test); GIE_EMPTY_VALUE when
 *                                               there is none or the flag is off;
 *                   flags                       the call's flags; reserved 0.
 *  which blocks   a block QUALIFIES iff it holds at least one known voxel (n_free + n_occupied + n_fnt > 0: whether a block without
 *                 one has been allocated is not observable) and lo_k <= k <= hi_k on every axis (INT32_MIN / INT32_MAX: open on
 *                 that side).
 *  list           *count = the number of qualifying blocks with n_fnt >= min_fnt, also when it exceeds max_records.  Exactly
 *                 min(count, max_records) records are written: distinct such blocks in unspecified order — which ones, when they do
 *                 not all fit, is unspecified too; entries beyond them are left as they were.  max_records == 0 with a NULL out only
 *                 counts.  A NULL count with a non-NULL out is allowed (the caller then cannot tell how many were written).
 *  grid           optional (NULL: none).  It needs a finite box, every side hi_k - lo_k + 1 <= 1024 and at most 2^24 cells in all;
 *                 cell ((k_z - lo_z) * ny + (k_y - lo_y)) * nx + (k_x - lo_x), x fastest.  EVERY cell is written: 0 where there is no
 *                 qualifying block, otherwise 1u << 31 | n_fnt << 20 | n_occupied << 10 | n_free (a count reaches 512, which ten
 *                 bits hold).  The grid ignores min_fnt.
 * GIE_ERR_INVALID: a NULL param; lo > hi on an axis; flags other than 0 or GIE_BLOCKS_DIST; min_fnt outside 0..512; max_records < 0;
 * non-zero reserved; a NULL out with max_records > 0; a NULL count together with a NULL out and a NULL grid; a grid with a box that
 * is open on a side, longer than 1024 blocks on a side or larger than 2^24 cells; a tiled mapper (its pool holds ghost blocks of
 * other tiles: refused, as by every planner section); in the _dev form a d_out that is not 16-byte aligned.  Nothing is written then.
 * The host form stages through the two scratch slots of the host forms and synchronises, like the display clouds.  The _dev form
 * takes DEVICE buffers and is enqueued on the mapper's stream with no host wait and no read-back: d_count and d_grid are zeroed on
 * the stream and written in place; at most two memsets and one launch, no grid barrier.  A call is legal wherever gie_query_global
 * is: before the first gie_set_pose too (an empty pool: count 0, a grid of zeros) and between gie_fuse and gie_merge of one update.
 * Map updates are not changed by it; a mapper that never calls it allocates and launches nothing (a _dev call with d_out but
 * without d_count uses the display clouds' counter word).
 * Cost: a key and 512 bytes per live block; GIE_BLOCKS_DIST 8 bytes more per FREE or FNT voxel; 32 bytes per record.
 * gie_profile_read has no entry for it. */
#define GIE_BLOCKS_DIST 1            /* flags: also reduce the distances */
typedef struct gie_blocks_param {    /* 48 bytes */
    int32_t lo[3], hi[3];   /* box of BLOCK coordinates (global voxel >> 3, arithmetic), both inclusive; INT32_MIN / INT32_MAX = open */
    int32_t flags;          /* 0 or GIE_BLOCKS_DIST */
    int32_t min_fnt;        /* 0..512: a RECORD is written only for a block with n_fnt >= min_fnt (the grid ignores it) */
    int32_t max_records;    /* >= 0: capacity of `out` */
    int32_t reserved[3];    /* 0 */
} gie_blocks_param;
typedef struct gie_block_summary {   /* 32 bytes */
    int32_t  key[3];        /* block coordinate */
    uint16_t n_free, n_occupied, n_fnt;   /* voxels of the block by type; UNKNOWN = 512 - their sum */
    uint16_t fnt_voxel;     /* least in-block index (x&7)*64 + (y&7)*8 + (z&7) (gie_stream_changed's order) of an FNT voxel; 0xffff: none */
    uint16_t free_voxel;    /* the same over FREE and FNT voxels; 0xffff: none */
    uint16_t flags;         /* the call's flags */
    int32_t  min_dist_sq;   /* GIE_BLOCKS_DIST: least dist_sq over the block's FREE / FNT voxels with 0 <= dist_sq < 900000; GIE_EMPTY_VALUE when there is none or the flag is off */
    int32_t  reserved;      /* 0 */
} gie_block_summary;
int gie_blocks_summary(gie_mapper *h, const gie_blocks_param *p, gie_block_summary *out, int32_t *count, uint32_t *grid);
int gie_blocks_summary_dev(gie_mapper *h, const gie_blocks_param *p, gie_block_summary *d_out, int32_t *d_count, uint32_t *d_grid);

/* ---- global block routes: face links between the blocks of everything mapped so far and a BFS field on the block grid.  The block
 * summaries above order far frontier by straight-line distance; this section says whether a block outside the local volume can be
 * reached through mapped space, how many blocks the route has and through which blocks it goes: the global counterpart of
 * gie_nf1_* and gie_ground_nf1_*.  No counterpart in the reference's code.
 *
 * Everything is an integer and exact.  r(g) = the record gie_query_global returns for global voxel g at the point of the mapper's
 * stream where gie_routes_compute* is enqueued.  passable(g) iff r(g).vox_type is GIE_VOX_FREE or GIE_VOX_FNT.  Block k holds the
 * voxels with g >> 3 == k (arithmetic shift on every axis: voxel -1 lies in block -1).  The call takes a finite box lo..hi of block
 * coordinates; its cells are nx x ny x nz, cell ((k_z - lo_z) * ny + (k_y - lo_y)) * nx + (k_x - lo_x), x fastest, as in
 * gie_blocks_summary's grid.  e_a = the unit step on axis a.
 *  node(k)       k lies inside the box and at least min_free of its 512 voxels are passable.
 *  pairs(k, a)   a in x, y, z: the number of the 64 voxel pairs (u, u + e_a) with u in block k at in-block coordinate 7 on axis a
 *                (so u + e_a lies in block k + e_a at coordinate 0) and both passable.
 *  link(k, a)    node(k), node(k + e_a) and pairs(k, a) >= min_open.  Links are undirected.  A link whose other end lies outside
 *                the box does not exist.
 *  frontier(k)   node(k) and the block has at least min_fnt FNT voxels.
 *  sources       the nodes among: the block of each goal point (metres, world frame: gie_pos2coord per axis, then >> 3; a point
 *                that is not finite or whose block lies outside the box is ignored, the mapping of gie_nf1_compute's goals) and,
 *                with GIE_ROUTES_FROM_FRONTIERS, every frontier block.  A goal on a block that is no node is ignored.
 *  steps(k)      int32: for a node joined to a source by a path of links, the number of links of the shortest such path (sources
 *                0); -1 for every other cell.
 *  cell byte     bit 0 node, bits 1 / 2 / 3 link(k, x / y / z), bit 4 frontier, bit 5 source; 0 for a cell without a node.
 * THE GRAPH IS OPTIMISTIC BY CONSTRUCTION: a block is one node, so a wall that runs through the INSIDE of a block does not cut it —
 * two faces of a block are joined whenever both have links, whether or not free space joins them inside.  That is the stated
 * approximation of a coarse router; the local stages (gie_nf1_*, gie_los_*) resolve the rest once the robot is there.  A wall lying
 * ON a block face (the voxels at coordinate 7 or those at coordinate 0 beyond it) is seen exactly.
 *
 *  gie_routes_compute*   builds cell bytes and field and keeps them, with their box, until the next compute.  n == 0 is valid; info
 *                        may be NULL.  n_reached counts the cells with steps >= 0, max_steps is the largest value (-1 without a
 *                        source).  n_links counts every link once.
 *  gie_read_routes*      the int32 field and the byte plane of the kept box (nx * ny * nz entries each); either pointer may be NULL,
 *                        not both.
 *  gie_routes_query*     steps of the blocks of n points (3 floats each, the goals' mapping): -1 for a point that is not finite,
 *                        outside the box, on a cell without a node or unreachable.  With the positions of
 *                        gie_blocks_summary's records this reads the route length to every far frontier block in one call.
 *  gie_routes_path*      one descent per start, in gie_nf1_path's form.  len = 0 when the start's block is outside the box (or the
 *                        point not finite) or has steps < 0.  Otherwise the blocks k_0 .. k_s with s = steps(k_0): k_{i+1} is the
 *                        first neighbour of k_i in the order -x +x -y +y -z +z that is joined to k_i by a link and has
 *                        steps(k_i) - 1.  path_key holds max_len block coordinates (3 int32) per start; min(len, max_len) are
 *                        written, entries beyond them are left as they were; len = s + 1 also when that exceeds max_len.
 * Size limit: with W = ceil(nx / 64) a bit plane has W * ny * nz 64-bit words; at most 16384 words (1 048 576 cells at nx = 128:
 * 128 x 128 x 64 blocks = 1024 x 1024 x 512 voxels).
 * GIE_ERR_INVALID, with nothing written: a NULL param; lo > hi on an axis; a side that is open (INT32_MIN / INT32_MAX); min_free
 * outside 1..512, min_open outside 1..64, min_fnt outside 1..512; non-zero reserved; unknown flags; n < 0; NULL points with n > 0; a
 * box over the size limit; read / query / path before the first compute, with max_len < 1 or with NULL arrays and n > 0; a tiled
 * mapper, for every call (its pool holds ghost blocks of other tiles).
 * The calls are legal wherever gie_query_global is: before the first gie_set_pose (an empty pool: every cell 0, the field -1) and
 * between gie_fuse and gie_merge of one update.  The stage writes nothing of the map; a mapper that never computes allocates and
 * launches nothing; memory is allocated at the first compute and grown when a later box is larger.  The host forms stage through
 * the scratch slots and synchronise; the _dev forms take DEVICE buffers and are enqueued on the mapper's stream with no host wait:
 * two memsets and three or four launches per compute (the propagation is ONE workgroup: no grid barrier, no cooperative launch).
 * Cost: a key and 512 bytes per live block inside the box plus 64 bytes of each of the three faces beyond it; 6 bytes per cell and
 * 5 bits per cell of planes.  gie_profile_read has no entry for it. */
#define GIE_ROUTES_FROM_FRONTIERS 1        /* flags: every frontier block is a source */
typedef struct gie_routes_param {          /* 48 bytes */
    int32_t lo[3], hi[3];                  /* finite box of BLOCK coordinates (global voxel >> 3, arithmetic), both inclusive */
    int32_t min_free, min_open, min_fnt;   /* 1..512, 1..64, 1..512 */
    int32_t flags;                         /* GIE_ROUTES_FROM_FRONTIERS */
    int32_t reserved[2];                   /* 0 */
} gie_routes_param;
typedef struct gie_routes_info {           /* 32 bytes */
    int32_t n_nodes, n_links, n_frontier, n_sources;
    int32_t n_reached, max_steps;          /* n_reached counts steps >= 0; max_steps is the largest value, -1 without a source */
    int32_t reserved[2];                   /* 0 */
} gie_routes_info;
int gie_routes_compute(gie_mapper *h, const float *goal_xyz, int n, const gie_routes_param *p, gie_routes_info *info);
int gie_routes_compute_dev(gie_mapper *h, const float *d_goal_xyz, int n, const gie_routes_param *p, gie_routes_info *d_info);
int gie_read_routes(gie_mapper *h, int32_t *steps, uint8_t *cells);
int gie_read_routes_dev(gie_mapper *h, int32_t *d_steps, uint8_t *d_cells);
int gie_routes_query(gie_mapper *h, const float *xyz, int n, int32_t *steps);
int gie_routes_query_dev(gie_mapper *h, const float *d_xyz, int n, int32_t *d_steps);
int gie_routes_path(gie_mapper *h, const float *start_xyz, int n, int max_len, int32_t *path_key, int32_t *len);
int gie_routes_path_dev(gie_mapper *h, const float *d_start_xyz, int n, int max_len, int32_t *d_path_key, int32_t *d_len);

/* ---- ground costmap: the footprint of a height band of the local volume and its exact 2-D distance transform, for ground and
 * planar robots (the reference's ugv_height set-ups: cfg/ugv_laser3D_params.yaml, cfg/scan2D_params.yaml).  A body that occupies a
 * band of z needs a 2-D grid — which cells are blocked, how far each is from the nearest blocked one — and neither the 3-D EDT nor
 * a z slice of it is that: the floor under the robot and a beam above it are obstacles one voxel away everywhere.  No counterpart
 * in the reference's code.
 *
 * Everything is over the local volume at the point of the mapper's stream where gie_ground_compute* is enqueued: type(v) is what
 * gie_read_local would return there, pvt what gie_get_pivot returns there.  The result is kept until the next compute and refers
 * to that pivot (as NF1's field); map updates do not change it.  Every value is an integer and exact.
 *  band          B = [max(z_lo, pvt_z), min(z_hi, pvt_z + Z - 1)] in GLOBAL z.  It may be empty: every column is then UNKNOWN.
 *  type(x, y)    from the voxels (x, y, z) with z in B: GIE_VOX_OCCUPIED if any of them is OCCUPIED; otherwise GIE_VOX_UNKNOWN if
 *                fewer than min_known of them are known (FREE, FNT or OCCUPIED); otherwise GIE_VOX_FNT if any of them is FNT;
 *                otherwise GIE_VOX_FREE.
 *  top(x, y)     the highest GLOBAL z in B at which the column is OCCUPIED, INT32_MIN for a column that is not OCCUPIED: a wall
 *                and a low kerb differ here.
 *  obstacle columns   the OCCUPIED columns; with GIE_GROUND_UNKNOWN_BLOCKS the UNKNOWN columns too.
 *  dist_sq(x, y) the exact squared Euclidean distance in the X x Y plane, in voxels, to the nearest obstacle column: 0 on obstacle
 *                columns, -1 when the rectangle holds no obstacle column.
 *  coc(x, y)     GLOBAL x, y of an obstacle column at exactly that distance (which one of several equally near is unspecified; an
 *                obstacle column is its own); GIE_EMPTY_VALUE each when there is none.
 *  counts        four int32, the number of columns of each type in GIE_VOX_* order (UNKNOWN, FREE, OCCUPIED, FNT).
 * CostMap (TYPE_EDT): hdr as gie_read_costmap fills it at the field's pivot, with z_size = 1 and z_origin = (float)z_lo * width (the
 *  caller's z_lo, converted as gie_read_costmap converts the pivot); payload of X * Y elements: d = sqrtf((float)dist_sq) in voxel
 *  units (sqrtf as in gie_read_sdf), (float)max_loc_dist_sq where dist_sq = -1 (gie_read_costmap's value for "no obstacle");
 *  o = type != UNKNOWN; s and the padding 0.  A consumer of the reference's cost_map topic takes it as a one-layer map.
 * Query at a point (metres, world frame): its cell is gie_pos2coord(p_k, w) - pvt_k for k = x, y (include/gie_math.h, the mapping
 *  of NF1's goals).  Inside the rectangle the record is the cell's, with inside = 1; outside it, or for a point that is not finite,
 *  dist_sq = -1, coc = GIE_EMPTY_VALUE, type = GIE_VOX_UNKNOWN, inside = 0.  n == 0 is valid.
 * Arguments: the planes of gie_read_ground* hold X * Y values each, x fastest (coc_xy two per cell); any may be NULL, not all.
 *  counts / d_counts may be NULL.  The host forms synchronise; the _dev forms take DEVICE buffers and are enqueued on the mapper's
 *  stream (gie_get_stream) with no host wait and no read-back.
 * GIE_ERR_INVALID, nothing written: a NULL handle or param; z_lo > z_hi; min_known < 1; an unknown flag bit or non-zero reserved;
 *  a compute before the first gie_set_pose; a tiled mapper (all eight refuse, as every planner section does); gie_read_ground*,
 *  gie_read_costmap_ground* or gie_ground_query* before the first compute; all four outputs of gie_read_ground* NULL; a NULL
 *  payload in gie_read_costmap_ground_dev; n < 0, or n > 0 with a NULL xy or out.
 * Memory: a mapper that never calls the section allocates and launches nothing.  The first compute allocates per CELL (x, y), not
 *  per voxel (gie_dalloc, freed by gie_destroy): dist_sq, top and the closest column (4 bytes each; the column as local x | y << 16),
 *  the type (1 byte), one bit row of obstacle columns per y padded to 64-bit words (8 * ceil(X/64) / X bytes per cell) and four
 *  counters: 13.125 bytes per cell when X is a multiple of 64, 3.4 MB for 512 x 512.  Whether a column is known or FNT is in its
 *  type byte, which every reader wants per cell; pass X's result is recomputed from the bit row where pass Y needs it.
 * Cost: a compute is one memset of the counters and two launches, without a grid barrier (it does not join the chain of
 *  grid-barrier launches).  The projection reads the type plane once over the band, 1 byte per voxel of X x Y x |B|, and nothing
 *  else of the map; the transform reads the bit rows and writes 8 bytes per cell.  With no obstacle column the transform returns at
 *  once on a device-side count and the readers write -1.
 * gie_profile_read: "ground" = compute and the exports, "ground_query" = the queries (the two entries before "cloud": a section's
 *  entries go in front of those of the sections before it; the map update's keep their indices). */
#define GIE_GROUND_UNKNOWN_BLOCKS 1      /* UNKNOWN columns are obstacles of the distance transform too */
typedef struct gie_ground_param {        /* 32 bytes */
    int32_t z_lo, z_hi;     /* GLOBAL voxel z, both inclusive (gie_cloud_param's convention); z_lo <= z_hi */
    int32_t min_known;      /* >= 1: a column with fewer known voxels inside the band is UNKNOWN */
    int32_t flags;          /* GIE_GROUND_* */
    int32_t reserved[4];    /* 0 */
} gie_ground_param;
typedef struct gie_ground_cell {         /* 16 bytes */
    int32_t dist_sq;
    int32_t coc_x, coc_y;   /* GLOBAL voxel x, y of a closest obstacle column; GIE_EMPTY_VALUE each when there is none */
    int8_t  type;           /* column type */
    uint8_t inside;         /* gie_ground_query only: the point lies inside the field's X x Y rectangle */
    uint8_t pad[2];         /* 0 */
} gie_ground_cell;
int gie_ground_compute(gie_mapper *h, const gie_ground_param *p, int32_t counts[4]);
int gie_ground_compute_dev(gie_mapper *h, const gie_ground_param *p, int32_t *d_counts);
int gie_read_ground(gie_mapper *h, int8_t *type, int32_t *dist_sq, int32_t *coc_xy, int32_t *top);
int gie_read_ground_dev(gie_mapper *h, int8_t *d_type, int32_t *d_dist_sq, int32_t *d_coc_xy, int32_t *d_top);
int gie_read_costmap_ground(gie_mapper *h, gie_seendist *payload, gie_costmap_hdr *hdr);
int gie_read_costmap_ground_dev(gie_mapper *h, gie_seendist *d_payload, gie_costmap_hdr *hdr);
int gie_ground_query(gie_mapper *h, const float *xy, int n, gie_ground_cell *out);
int gie_ground_query_dev(gie_mapper *h, const float *d_xy, int n, gie_ground_cell *d_out);

/* ---- ground navigation function: NF1 and its descent paths on the ground costmap — the planner of the configurations that set
 * ugv_height.  gie_nf1_compute is no use to them for the reason the ground costmap exists: in the volume the floor is an obstacle
 * one voxel away everywhere, so no useful clearance leaves anything traversable at floor level.  No counterpart in the reference.
 *
 * Everything is over the ground field that is valid where gie_ground_nf1_compute* is enqueued: type(c), dist_sq(c) and the pivot
 * are that field's (gie_read_ground*).  Every value is an integer and exact.
 *  traversable(c)  type(c) is FREE or FNT (or UNKNOWN, with GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE), and dist_sq(c) == -1 or
 *                  dist_sq(c) >= clearance_sq (squared cells).  dist_sq is the field's own: computed with GIE_GROUND_UNKNOWN_BLOCKS
 *                  an UNKNOWN column is an obstacle column at distance 0 and is traversable at clearance_sq == 0 only.
 *  sources         the traversable cells among: the cell of each goal (metres, world frame, two floats per goal), which is
 *                  gie_pos2coord(g_k, w) - pvt_k for k = x, y — gie_ground_query's mapping; goals outside the rectangle or not
 *                  finite are ignored — and, with GIE_GROUND_NF1_FROM_FRONTIERS, every FNT cell.  n == 0 is valid.  *n_sources =
 *                  the number of distinct source cells (n_sources / d_n_sources may be NULL).
 *  nf1(c)          the number of steps of the shortest 4-connected path of traversable cells inside the rectangle from c to a
 *                  source: 0 on sources, -1 where there is no such path (cells that are not traversable included).  X * Y int32, x
 *                  fastest.
 *  path            for each of n start points (the goals' mapping): len = 0 for a start outside the rectangle, not finite, or with
 *                  nf1 < 0.  Otherwise v_0 = the start's cell and v_{i+1} = the first 4-neighbour of v_i in the order -x +x -y +y
 *                  whose value is nf1(v_i) - 1, down to a source; len = nf1(start) + 1 also when that exceeds max_len.  path_xy
 *                  holds max_len points per start, each two int32, GLOBAL x, y; exactly min(len, max_len) of them are written, the
 *                  rest is left as it was.
 *  CostMap         the header gie_read_costmap_ground fills (z_size 1, z_origin from the ground field's z_lo) with type = 2
 *                  (TYPE_NF1); payload of X * Y elements: d = (float)nf1, -1.0f where nf1 is -1; o = type != UNKNOWN; s and the
 *                  padding 0.
 * Lifetime: the field is kept until the next gie_ground_nf1_compute* and refers to the ground field's pivot; a map update does
 *  not change it.  A later gie_ground_compute* invalidates it — the readers, the paths and the CostMap then return GIE_ERR_INVALID
 *  until the next gie_ground_nf1_compute*: no copy of the ground field's type plane is kept.
 * GIE_ERR_INVALID, nothing written: a NULL handle or param; clearance_sq < 0; an unknown flag bit or non-zero reserved; n < 0, or
 *  n > 0 with a NULL array (goals; starts, path_xy or len); max_len < 1; a compute before a ground field exists; a read, path or
 *  CostMap before the first compute or after an invalidation; a NULL output in gie_read_ground_nf1_dev, a NULL payload in
 *  gie_read_costmap_ground_nf1_dev; a tiled mapper (all eight refuse, as every planner section does).
 * The host forms synchronise; the _dev forms take DEVICE buffers and are enqueued on the mapper's stream (gie_get_stream) with no
 *  host wait and no read-back.
 * Memory: a mapper that never calls the section allocates and launches nothing.  The first compute allocates per CELL (gie_dalloc,
 *  freed by gie_destroy): the field (4 bytes), two bit planes with rows padded to 64-bit words — blocked or visited, and the
 *  frontier — and four control words: 4.25 bytes per cell when X is a multiple of 64, 1.1 MB for 512 x 512.
 * Cost: a compute is at most three launches: the bit planes (one pass over the ground field's type and dist_sq, 5 bytes per cell),
 *  the goals, and the propagation — ONE workgroup that runs every BFS level up to a workgroup barrier, on bit planes it holds
 *  in the LDS of its compute unit when three — frontier, next frontier, blocked — fit 144 KiB (ceil(X/64) * Y <= 6144 words: 512 x 768
 *  and everything smaller), on the two planes in global memory otherwise; which, the size alone decides.  No grid barrier: the launch is no member of the chain of
 *  grid-barrier launches, needs no co-residency and has no timeout path — gie_nf1_compute's GIE_ERR_TIMEOUT cannot occur; the
 *  number of levels is bounded by X * Y on the device.  A level costs the workgroup one pass over the two planes and a 4-byte
 *  store per cell that gets its value.
 * gie_profile_read: "ground_nf1" = compute, exports and paths (the entry in front of "ground"). */
#define GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE 1    /* UNKNOWN cells may be traversed (their dist_sq still decides) */
#define GIE_GROUND_NF1_FROM_FRONTIERS 2         /* every traversable FNT cell is a source */
typedef struct gie_ground_nf1_param {   /* 32 bytes */
    int32_t clearance_sq;   /* >= 0, squared cells: dist_sq of a traversable cell is at least this (or -1) */
    int32_t flags;          /* GIE_GROUND_NF1_* */
    int32_t reserved[6];    /* 0 */
} gie_ground_nf1_param;
int gie_ground_nf1_compute(gie_mapper *h, const float *goal_xy, int n, const gie_ground_nf1_param *p, int32_t *n_sources);
int gie_ground_nf1_compute_dev(gie_mapper *h, const float *d_goal_xy, int n, const gie_ground_nf1_param *p, int32_t *d_n_sources);
int gie_read_ground_nf1(gie_mapper *h, int32_t *nf1);
int gie_read_ground_nf1_dev(gie_mapper *h, int32_t *d_nf1);
int gie_ground_nf1_path(gie_mapper *h, const float *start_xy, int n, int max_len, int32_t *path_xy, int32_t *len);
int gie_ground_nf1_path_dev(gie_mapper *h, const float *d_start_xy, int n, int max_len, int32_t *d_path_xy, int32_t *d_len);
int gie_read_costmap_ground_nf1(gie_mapper *h, gie_seendist *payload, gie_costmap_hdr *hdr);
int gie_read_costmap_ground_nf1_dev(gie_mapper *h, gie_seendist *d_payload, gie_costmap_hdr *hdr);

/* ---- ground line of sight: straight segments and any-angle paths on the ground costmap — the ground counterparts of the segment
 * checks of "line of sight" and of "path shortcutting".  Those two read the opaque plane of gie_los_prepare, which is built from
 * the volume: there the floor is an obstacle one voxel away everywhere (why the ground costmap exists).  Here a disc robot's
 * straight move is tested against the ground field, and gie_ground_nf1_path's 4-connected staircase becomes the few straight legs
 * a controller can follow.  No counterpart in the reference's code.
 *
 * Every call refers to the ground field that is valid where the call is enqueued: type(c), dist_sq(c) and the pivot are that field's
 * (gie_read_ground*).  There is no prepare call and no kept result: a later gie_ground_compute* simply makes later calls see the
 * new field; a map update changes nothing, because it does not change the ground field; the ground navigation function is not
 * needed and not touched.  Every value but `length` is an integer and exact.
 *  blocked(c)    c is not traversable by the ground navigation function's rule: traversable(c) iff type(c) is FREE or FNT (or
 *                UNKNOWN, with GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE), and dist_sq(c) == -1 or dist_sq(c) >= clearance_sq (squared
 *                cells).  A field without an obstacle column has dist_sq == -1 everywhere: every clearance passes.  The robot's
 *                disc is swept along a line by that rule: a cell of the line closer than the radius to an obstacle column is blocked.
 *  cell line     L2(a, b), for local cells a and b: the voxel line of "line of sight" on two axes — the cells whose square shares
 *                a piece of POSITIVE length with the straight segment between the two cell centres, in the order of those pieces
 *                from a to b.  L2(a, a) = (a).  The walk: with n_k = |b_k - a_k|, crossing j (1..n_k) of axis k lies at
 *                t = (2j - 1) / (2 n_k); take the smaller pending t and step BOTH axes when they tie, until none is pending.
 *                (2 j_x - 1) * n_y against (2 j_y - 1) * n_x decides the order, exactly in 32-bit integers (gie_create keeps every
 *                side <= 1024).  L2(b, a) is L2(a, b) reversed; no cell repeats; 1 + max(n_x, n_y) <= len <= 1 + n_x + n_y;
 *                L2(a, b) is L((a, 0), (b, 0)) of "line of sight" without the third coordinate.
 *                A tie is a diagonal move through a corner of the grid: the two cells that touch the line only at that corner
 *                are not on it, so the line passes BETWEEN two corner-touching cells whatever they hold.  With clearance_sq >= 2
 *                that is harmless: a cell beside an obstacle column (dist_sq 1) is then blocked itself, and a diagonal move between
 *                two obstacle columns has both its ends blocked.  With clearance_sq 0 or 1 a line may slip between two obstacle
 *                columns that touch at a corner.
 *  segment       a pair of points (metres, world frame, two floats each), each mapped as in gie_ground_query:
 *                gie_pos2coord(p_k, w) - pvt_k for k = x, y.  Result, one gie_ground_hit per segment:
 *                  first        index along L2(a, b) of the first blocked cell (a has index 0); -1 when none is blocked; -2 when
 *                               an endpoint is not finite or lies outside the field's rectangle (every other field is then 0);
 *                  len          the number of cells of L2(a, b);
 *                  hit          the first blocked cell, GLOBAL cell coordinates (local + pivot); b's when first == -1;
 *                  min_dist_sq  the minimum of dist_sq over the cells of index 0 .. first (all of the line when first == -1), the
 *                               values gie_read_ground returns: -1 on a field without an obstacle column;
 *                  reserved     0.
 *  shortcut input  the buffers of gie_ground_nf1_path*: n paths of max_len points (2 int32 each, GLOBAL cell coordinates), len[i]
 *                as that call left it: path i has m = min(max(len[i], 0), max_len) points v_0 .. v_{m-1}.  Any polyline of cells is
 *                legal: it need not be 4-connected or come from NF1, points may repeat, lie outside the field or be any int32
 *                (local = global - pivot is computed in 64 bits).
 *  Clear(a, b)   a and b are inside the field's rectangle and no cell of L2(a, b), both ends included, is blocked.
 *  waypoints     indices k_0 = 0 < k_1 < .. < k_T = m - 1.  While k_t < m - 1, with K = lookahead:
 *                  J = { j : k_t < j <= min(k_t + K, m - 1) and Clear(v_{k_t}, v_j) };  k_{t+1} = max J,
 *                or, when J is empty, k_{t+1} = k_t + 1 and that leg is FORCED: the path stays connected and the caller learns that
 *                it is not valid there.  Visibility along a path is not monotone (a pillar's shadow hides a stretch of points and
 *                lets the ones behind it through): max J is the largest clear index of the whole window, not the last before the
 *                first blocked one.  count = T + 1; 0 when m = 0.
 *  gie_ground_waypoint  record t: xy = v_{k_t} as given, index = k_t, reserved = 0.
 *                  t = 0: forced = 0; min_dist_sq = dist_sq(v_0) when v_0 is inside the rectangle, otherwise -2.
 *                  a clear leg: forced = 0; min_dist_sq = the minimum of dist_sq over all cells of L2(v_{k_{t-1}}, v_{k_t}).
 *                  a forced leg: forced = 1; min_dist_sq = -2.  (-1 is a legal distance — no obstacle column — so -2 marks
 *                  "no value".)
 *  gie_shortcut_info  the record of "path shortcutting", reused: count as above, even when it exceeds max_wp; forced = the number
 *                of forced legs; length = a float sum, started at 0.0f and accumulated in leg order t = 1 .. T: each CLEAR leg adds
 *                sqrtf((float)(dx^2 + dy^2)) of its two ends (an exact integer below 2^22; sqrtf as in gie_read_sdf), a forced leg
 *                adds nothing.  The unit is cells.
 *  capacity      wp holds max_wp records per path; only the first min(count, max_wp) of a path are written (the convention of
 *                gie_ground_nf1_path's len > max_len), entries beyond them are left as they are.  info is complete whatever max_wp
 *                is.  Shortcutting a path of gie_ground_nf1_path with the clearance_sq and UNKNOWN flag of its
 *                gie_ground_nf1_compute has no forced leg: consecutive path cells are traversable neighbours.
 * GIE_ERR_INVALID, nothing written: a NULL handle; a tiled mapper (all four refuse, as every planner section does); no ground field
 *  yet; a NULL param; clearance_sq < 0; a flag other than GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE; non-zero reserved; n < 0; n > 0 with a
 *  NULL input (a_xy, b_xy; path_xy, len) or, for segments, a NULL out; max_len < 1; lookahead outside 1..4096; max_wp < 0; wp NULL
 *  with max_wp > 0; wp and info both NULL.  n == 0 is valid and launches nothing.
 * The host forms stage through the two scratch slots of the host forms and synchronise; gie_ground_shortcut hands the entries of
 *  wp beyond a path's records back as they were.  The _dev forms take DEVICE buffers and are enqueued on the mapper's stream
 *  (gie_get_stream) with no host wait, no read-back and no grid barrier.
 * Memory: a mapper that never calls the section allocates and launches nothing.  The first call allocates one bit plane of blocked
 *  cells with rows padded to 64-bit words (8 * ceil(X/64) / X bytes per cell: 32 KiB for 512 x 512; gie_dalloc, freed by
 *  gie_destroy), of which no reader may assume anything between calls.
 * Cost: a call is two launches: the blocked plane (one pass over the ground field's type and dist_sq, 5 bytes per cell) and the
 *  query — a lane per segment, or a wave per path (a leg costs its window's lines in chunks of 64 from the far end, up to the first
 *  chunk with a clear one; a point outside the rectangle or in a blocked cell costs nothing).
 * gie_profile_read: counted under "ground_query". */
#define GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE 1    /* UNKNOWN cells are not blocked by their type (their dist_sq still decides) */
typedef struct gie_ground_los_param {   /* 16 bytes */
    int32_t clearance_sq;   /* >= 0, squared cells: dist_sq of a cell that is not blocked is at least this (or -1) */
    int32_t flags;          /* GIE_GROUND_LOS_* */
    int32_t reserved[2];    /* 0 */
} gie_ground_los_param;
typedef struct gie_ground_hit {         /* 24 bytes */
    int32_t first;
    int32_t len;
    int32_t hit[2];
    int32_t min_dist_sq;
    int32_t reserved;       /* 0 */
} gie_ground_hit;
typedef struct gie_ground_shortcut_param {   /* 32 bytes */
    int32_t lookahead;      /* K in 1..4096: a leg may reach at most K path points ahead */
    int32_t max_wp;         /* >= 0: capacity of the waypoint array, per path */
    int32_t clearance_sq;   /* as gie_ground_los_param */
    int32_t flags;          /* GIE_GROUND_LOS_* */
    int32_t reserved[4];    /* 0 */
} gie_ground_shortcut_param;
typedef struct gie_ground_waypoint {    /* 24 bytes */
    int32_t xy[2];          /* the path point, GLOBAL cell coordinates, copied from the input */
    int32_t index;          /* its index in the input path */
    int32_t min_dist_sq;    /* squared cells; -2: a forced leg, or a first point outside the rectangle */
    int32_t forced;         /* 1: the leg that ends here is not a clear line */
    int32_t reserved;       /* 0 */
} gie_ground_waypoint;
int gie_ground_segments(gie_mapper *h, const float *a_xy, const float *b_xy, int n, const gie_ground_los_param *p, gie_ground_hit *out);
int gie_ground_segments_dev(gie_mapper *h, const float *d_a_xy, const float *d_b_xy, int n, const gie_ground_los_param *p,
                            gie_ground_hit *d_out);
int gie_ground_shortcut(gie_mapper *h, const int32_t *path_xy, const int32_t *len, int n, int max_len,
                        const gie_ground_shortcut_param *p, gie_ground_waypoint *wp, gie_shortcut_info *info);
int gie_ground_shortcut_dev(gie_mapper *h, const int32_t *d_path_xy, const int32_t *d_len, int n, int max_len,
                            const gie_ground_shortcut_param *p, gie_ground_waypoint *d_wp, gie_shortcut_info *d_info);

/* ---- ground frontier clusters: the connected components of the ground field's FNT cells, filtered by size, each with a goal a
 * ground robot can drive to, and the route length from the robot to each of them — the goal selection of an exploration loop
 * ("which frontiers exist, how large are they, where do I drive for each, how far is it").  "frontier clusters" above does not
 * serve a ground robot for the reason the ground costmap exists: in the volume the floor is an obstacle one voxel away
 * everywhere, so FNT voxels at floor level fail every useful clearance, and the 3-D components are sheets, not the 2-D arcs a
 * ground planner reasons about.  No counterpart in the reference's code.
 *
 * Everything is over the ground field that is valid where gie_ground_frontier_compute* is enqueued: type(c), dist_sq(c) and the
 * pivot are that field's (gie_read_ground*).  id(c) = y * X + x is the local cell index.  Every value is an integer and exact; the
 * floats are derived from the integers in the order of operations stated here.  w = voxel_width.
 *  member(c)     type(c) == GIE_VOX_FNT, and dist_sq(c) == -1 or dist_sq(c) >= clearance_sq (squared cells): the ground navigation
 *                function's traversable rule restricted to FNT cells, so with equal clearance_sq every member is a legal source or
 *                goal of gie_ground_nf1_compute.
 *  adjacent      two distinct members that differ by at most 1 in x and in y (connectivity = 8), or that are edge neighbours
 *                (connectivity = 4).  Any other value: GIE_ERR_INVALID.
 *  component     a class of the transitive closure of `adjacent` inside the rectangle.  Its label is the smallest id of its members,
 *                its size the number of members.  Both are independent of any schedule.
 *  kept          size >= min_size: the noise filter.
 *  label plane   X * Y int32, x fastest: -1 not a member; -2 member of a component that is not kept; otherwise the label.
 *  cluster record  one gie_ground_frontier_cluster per kept component, in ascending order of label.
 *                centroid_k = ((float)((double)sum_k / (double)size) + (float)pvt_k) * w, in this order of operations.
 *                rep: with c_k = (2 * sum_k + size) / (2 * size) (integer division: the centroid rounded half up to a cell), the
 *                member that minimises |v - c|^2 (integers), ties to the smaller id.  The centroid of an arc is usually not a
 *                member and may lie in an obstacle column; rep always is a member.  rep_dist_sq = dist_sq(rep), the value
 *                gie_read_ground returns (-1 on a field without an obstacle column): the room the robot has at its goal.
 *                These are the rules of "frontier clusters" in two dimensions.
 *  capacity      n_clusters is the number of KEPT components even when it exceeds max_clusters; only the first max_clusters
 *                records (ascending label) are produced.  n_cells = members in kept components.  The label plane is complete
 *                whatever the capacity.  d_counts (device, 2 int32, may be NULL) = { n_clusters, n_cells }; n_clusters / n_cells
 *                of the host form may be NULL.
 *  readers       gie_read_ground_frontier_clusters*: out and goal_xy hold max_clusters (of the compute) entries, either may be
 *                NULL, not both.  out: the records produced; entries beyond them are left as they are.  goal_xy (2 floats per
 *                entry): (float)rep_k * w for the records produced, NaN for the rest — so the whole array can be handed to
 *                gie_ground_nf1_compute_dev and gie_ground_nf1_query_dev with n = max_clusters without the host ever learning the
 *                count (both ignore points that are not finite).  gie_pos2coord((float)rep_k * w, w) = floorf(p / w + 0.5f) gives
 *                rep_k back while |rep_k| < 2^20: product and quotient are each off by at most a few ulp of a value below 2^20
 *                (3 * 2^-4 of a cell in all), inside the half-cell margin.  *n_clusters as the compute's (may be NULL).
 *                gie_read_ground_frontier_labels*: the label plane.
 *  gie_ground_nf1_query*  for each of n points (metres, world frame, two floats each): its cell by gie_ground_query's mapping,
 *                gie_pos2coord(p_k, w) - pvt_k; steps = the value of the current ground navigation function at that cell, -1 for a
 *                point outside the rectangle or not finite.  n == 0 is valid.  Refused exactly where gie_read_ground_nf1* is: no
 *                field yet, or the field invalidated by a later gie_ground_compute*.  Ground NF1 is symmetric: ONE field whose
 *                only goal is the robot, gathered at the clusters' goal array, gives the route length from the robot to every
 *                cluster (-1: not reachable, or the NaN tail of the array) — instead of one compute per candidate goal.
 * Lifetime: the clusters are kept until the next gie_ground_frontier_compute* and refer to the ground field's pivot; a map update
 *  does not touch them.  A later gie_ground_compute* invalidates them (one flag, as for the ground navigation function): the three
 *  readers then return GIE_ERR_INVALID until the next gie_ground_frontier_compute*.
 * GIE_ERR_INVALID, nothing written: a NULL handle or param; clearance_sq < 0; min_size < 1; a connectivity other than 4 and 8;
 *  max_clusters < 0; non-zero flags or reserved; a compute before a ground field exists; a reader before the first compute or after
 *  an invalidation; both outputs of the cluster reader NULL; a NULL plane in the label readers; n < 0, or n > 0 with a NULL array;
 *  a tiled mapper (all eight refuse, as every planner section does).
 * The host forms synchronise; the _dev forms take DEVICE buffers and are enqueued on the mapper's stream (gie_get_stream) with no
 *  host wait and no read-back.
 * Memory: a mapper that never calls the section allocates and launches nothing.  The first compute allocates per CELL (gie_dalloc,
 *  freed by gie_destroy): the union-find forest and the sizes (8 bytes), two bit planes with rows padded to 64-bit words — members,
 *  kept roots — and 8 bytes per such word (0.375 bytes per cell when X is a multiple of 64): 2.2 MB for 512 x 512; and 64 bytes per
 *  record of the largest max_clusters asked for.
 * Cost: a compute is one memset and a fixed sequence of about a dozen launches whatever the data (three fewer with max_clusters == 0),
 *  none with a grid barrier: it does not join the chain of grid-barrier launches and has no timeout path; no loop of the host's, no
 *  read-back.  The member plane is one pass over the ground field's type and dist_sq (5 bytes per cell); everything after it works
 *  on 64-bit words of that plane.  The statistics are integer atomics, one set per (64 x 64 tile, component) and not per member
 *  or run, so a result is bit-identical from run to run and one large component is no hot spot.  The gather is one launch, a lane
 *  per point.
 * gie_profile_read: "ground_frontier" = the compute and the three readers, the entry directly in front of "ground_nf1"; it is
 *  listed once the mapper has called gie_ground_frontier_compute* — the profile of a mapper that never calls the section is the
 *  list as it was.  The gather is counted under "ground_nf1". */
typedef struct gie_ground_frontier_cluster {   /* 64 bytes */
    int32_t label;          /* smallest local cell index y * X + x of a member */
    int32_t size;
    int32_t lo[2], hi[2];   /* bounding box, GLOBAL x, y (local + pivot), both inclusive */
    int32_t rep[2];         /* representative member, GLOBAL x, y */
    float   centroid[2];    /* metres, world frame */
    int64_t sum[2];         /* sums of the members' LOCAL x, y  (offset 40) */
    int32_t rep_dist_sq;    /* the ground field's dist_sq at rep (-1: no obstacle column) */
    int32_t reserved;       /* 0 */
} gie_ground_frontier_cluster;
typedef struct gie_ground_frontier_param {     /* 32 bytes */
    int32_t clearance_sq;   /* >= 0, squared cells */
    int32_t min_size;       /* >= 1 */
    int32_t connectivity;   /* 4 or 8 */
    int32_t max_clusters;   /* >= 0 */
    int32_t flags;          /* 0 */
    int32_t reserved[3];    /* 0 */
} gie_ground_frontier_param;
int gie_ground_frontier_compute(gie_mapper *h, const gie_ground_frontier_param *p, int32_t *n_clusters, int32_t *n_cells);
int gie_ground_frontier_compute_dev(gie_mapper *h, const gie_ground_frontier_param *p, int32_t *d_counts);   /* {n_clusters, n_cells}, may be NULL */
int gie_read_ground_frontier_clusters(gie_mapper *h, gie_ground_frontier_cluster *out, float *goal_xy, int32_t *n_clusters);
int gie_read_ground_frontier_clusters_dev(gie_mapper *h, gie_ground_frontier_cluster *d_out, float *d_goal_xy, int32_t *d_n_clusters);
int gie_read_ground_frontier_labels(gie_mapper *h, int32_t *labels);
int gie_read_ground_frontier_labels_dev(gie_mapper *h, int32_t *d_labels);
int gie_ground_nf1_query(gie_mapper *h, const float *xy, int n, int32_t *steps);
int gie_ground_nf1_query_dev(gie_mapper *h, const float *d_xy, int n, int32_t *d_steps);

/* ---- ground cost matrix: the route lengths among up to 256 points on the ground costmap (the robot and the goals of the ground
 * frontier clusters, say) — the input of every tour-based explorer of a ground robot: in which order to visit the clusters.  It is
 * "cost matrix" below in two dimensions, on the ground navigation function's rules; that section does not serve a ground robot for
 * the reason the ground costmap exists.  n calls of gie_ground_nf1_compute* and gie_ground_nf1_query* would give the same numbers
 * one after the other, each on one compute unit, and each would overwrite the ONE ground navigation function the robot's own plan
 * needs; here the n searches are the n workgroups of one launch and no field is written.  No counterpart in the reference's code.
 *
 * Everything is over the ground field that is valid where gie_ground_costmat_compute* is enqueued: type(c), dist_sq(c) and the pivot
 * are that field's (gie_read_ground*).  Every value is an integer and exact.  w = voxel_width.
 *  traversable(c)  the ground navigation function's rule with this call's clearance_sq (squared cells): type(c) is FREE or FNT (or
 *                  UNKNOWN, with GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE), and dist_sq(c) == -1 or dist_sq(c) >= clearance_sq.
 *                  GIE_GROUND_NF1_UNKNOWN_TRAVERSABLE is the only legal flag: GIE_GROUND_NF1_FROM_FRONTIERS has no meaning here
 *                  and is GIE_ERR_INVALID.
 *  cell(i)         of point i (metres, world frame, two floats), gie_ground_query's mapping: gie_pos2coord(p_k, w) - pvt_k.  The
 *                  point is VALID when it is finite, inside the rectangle and its cell traversable.  valid[i] = 1 or 0 (valid may
 *                  be NULL).
 *  cost            n x n int32, row-major.  cost[i][j] = the number of steps of the shortest 4-connected path from cell(i) to
 *                  cell(j) whose every cell is traversable and inside the rectangle; 0 when the cells coincide (i = j included);
 *                  -1 when either point is invalid or there is no such path.  The matrix is symmetric, the rows and columns of
 *                  invalid points are all -1, two points on one cell have identical rows.  By definition cost[i][j] is what
 *                  gie_ground_nf1_query returns at point i on the field gie_ground_nf1_compute gives for the single goal j with
 *                  the same clearance_sq and flags.
 * Arguments: 0 <= n <= GIE_GROUND_COSTMAT_MAX_POINTS; n == 0 is valid, writes nothing and launches nothing.
 * GIE_ERR_INVALID, nothing written: a NULL handle; a tiled mapper (as every planner section: the searches would stop at the tile's
 *  faces); a call before a ground field exists; a NULL p; clearance_sq < 0; an unknown flag, or GIE_GROUND_NF1_FROM_FRONTIERS;
 *  non-zero reserved; n outside the range; n > 0 with a NULL xy or cost.
 * The goal array gie_read_ground_frontier_clusters_dev writes (NaN in its unused entries) can stand behind a robot position in one
 *  buffer and be handed over as it is: max_clusters + 1 points, the NaN ones invalid.  The host never learns a count.
 * State: nothing is kept for later readers; the result is complete when the call's work is done.  The call neither reads, writes nor
 *  invalidates the current ground navigation function or the ground frontier clusters, and a map update does not touch it.
 * The host form stages through the export buffers and synchronises.  The _dev form takes DEVICE buffers and is enqueued on the
 *  mapper's stream (gie_get_stream) with no host wait and no read-back.
 * Propagation: one launch of n workgroups of 1024 threads, workgroup i the whole search from point i: the ground navigation
 *  function's level loop on three bit planes in the LDS of one compute unit (144 KiB: one workgroup per compute unit, 256 points
 *  occupy the chip once), one workgroup barrier per level, without the stores of a field: a search only notes the level at which
 *  the other points' bits enter its frontier.  It ends when a level adds nothing, or one level after its last valid target was
 *  found; the matrix is the same either way.  A field beyond the LDS budget (ceil(X/64) * Y > 6144 words, 1024 x 1024 say) runs the
 *  same loop with two of the planes in global memory, a pair PER SOURCE, and two barriers per level.  No grid barrier and no
 *  co-residency: the launch does not join the chain of grid-barrier launches and has no timeout path; the level count is bounded
 *  by X * Y.  Only integers, no atomics, a row is written by one workgroup only: a result is bit-identical from run to run.
 * Memory: a mapper that never calls the section allocates and launches nothing.  The first call allocates one bit plane with rows
 *  padded to 64-bit words (gie_dalloc, freed by gie_destroy; 32 KiB for 512 x 512); the first call on a field beyond the LDS budget
 *  two such planes per point, for the largest n asked for (64 MiB for 1024 x 1024 and 256 points).
 * gie_profile_read: counted under "ground_nf1"; no entry of its own. */
#define GIE_GROUND_COSTMAT_MAX_POINTS 256
int gie_ground_costmat_compute(gie_mapper *h, const float *xy, int n, const gie_ground_nf1_param *p, int32_t *cost, uint8_t *valid);
int gie_ground_costmat_compute_dev(gie_mapper *h, const float *d_xy, int n, const gie_ground_nf1_param *p, int32_t *d_cost, uint8_t *d_valid);

/* ---- ground view gain: how many cells of the ground field a sensor would see from each of n candidate poses — the gain half of a
 * ground robot's exploration utility, beside the route costs of "ground frontier clusters" and "ground cost matrix".  It is the view
 * gain of "line of sight" in two dimensions; that call does not serve a ground robot for the reason the ground costmap exists: it
 * reads the opaque plane of gie_los_prepare, which is built from the volume, where the floor is opaque one voxel below every line.
 * No counterpart in the reference's code.
 *
 * Every call refers to the ground field that is valid where the call is enqueued: type(c) and the pivot are that field's
 * (gie_read_ground*).  There is no prepare call and no kept result (the rule of "ground line of sight"): a later gie_ground_compute*
 * makes later calls see the new field, a map update changes nothing, the ground navigation function is neither needed nor touched.
 * Everything is an integer or one float operation on exact integers.  w = voxel_width.
 *  views         two plain arrays: xy, 2 floats per view (metres, world frame), and normals, 2 * n_planes int32 per view, x then y
 *                per plane; normals is not read (and may be NULL) when n_planes == 0.  The goal array of
 *                gie_read_ground_frontier_clusters_dev, NaN tail included, can be handed over as d_xy unchanged.
 *  p             the cell of a view's xy, gie_ground_query's mapping: gie_pos2coord(xy_k, w) - pvt_k.
 *  opaque(c)     type(c) == GIE_VOX_OCCUPIED, or type(c) == GIE_VOX_UNKNOWN with GIE_GROUND_VIEW_UNKNOWN_OPAQUE.  dist_sq has no part
 *                in it: sight is not clearance.
 *  candidate     cell v is a CANDIDATE iff
 *                  v is inside the rectangle and v != p;
 *                  with d = v - p, rmin = r_min / w and rmax = r_max / w (float): (float)|d|^2 >= rmin * rmin and
 *                  (float)|d|^2 <= rmax * rmax (|d|^2 is an exact integer below 2^21: one float product and one comparison on
 *                  each side; whatever box an implementation bounds the candidates with, this test decides alone);
 *                  the sector: n_planes == 1: normal_0 . d >= 0; n_planes == 2: both, or with GIE_GROUND_VIEW_UNION at least one of
 *                  them (a sector wider than 180 degrees).  A normal component has magnitude <= 32767: the dot product is an exact
 *                  int32.  A zero normal holds for every d.
 *  visible       a candidate is VISIBLE iff no cell of L2(p, v) other than v itself is opaque; L2 is the cell line of "ground line
 *                of sight", tie rule included (a line slips between two corner-touching cells).  p's own opacity is ignored, v may
 *                be anything.
 *  gie_view_score  the record of "line of sight", reused: unknown / frontier / occupied = the visible candidates of that column
 *                type, candidates = all candidates; all four are -1 when xy is not finite or lies outside the rectangle.  The
 *                counts are sums: they depend on no schedule.
 *  mask          one view: X * Y bytes, x fastest: 0 not a candidate, 1 a hidden candidate, 2 a visible candidate; the byte at p
 *                itself is 0.  An invalid view: the mask is all 0 and the score -1.  score may be NULL.
 * GIE_ERR_INVALID, nothing written: a NULL handle or param; a call before the first gie_ground_compute*; a tiled mapper (as every
 *  planner section); r_min or r_max not finite, r_min < 0, r_min > r_max (r_max may be anything finite); n_planes outside 0..2; an
 *  unknown flag, GIE_GROUND_VIEW_UNION with n_planes != 2, non-zero reserved; n < 0; n > 0 with a NULL xy or out; normals NULL with
 *  n_planes > 0; a NULL mask; in the host forms only, a normal component beyond +-32767 — the _dev forms never read the arrays on the
 *  host: such a view scores -1 there.  n == 0 is valid and launches nothing; n has no upper limit.
 * The host forms stage through the two scratch slots of the host forms and synchronise.  The _dev forms take DEVICE buffers and are
 *  enqueued on the mapper's stream (gie_get_stream) with no host wait and no read-back.  Every call is a fixed sequence of launches,
 *  none with a grid barrier.
 * Memory: a mapper that never calls the section allocates and launches nothing.  The first call allocates one bit plane of opaque
 *  cells with rows padded to 64-bit words (32 KiB for 512 x 512, 128 KiB for 1024 x 1024; gie_dalloc, freed by gie_destroy), of
 *  which no reader may assume anything between calls.
 * Cost: a call is two launches: the opaque plane (one pass over the type plane, which also writes the n scores' zeros and the mask's)
 *  and the gain.  A workgroup of the gain takes a strip of a view's candidate rows, copies the opaque words between the view's cell
 *  and its strip into LDS (at most the whole plane, 128 KiB) and walks each candidate's line there: a step is an LDS bit test.
 * gie_profile_read: counted under "ground_query". */
#define GIE_GROUND_VIEW_UNKNOWN_OPAQUE 1   /* UNKNOWN columns block sight too */
#define GIE_GROUND_VIEW_UNION          2   /* n_planes == 2: a cell in EITHER half plane is inside (a sector wider than 180 degrees) */
typedef struct gie_ground_view_param {     /* 32 bytes */
    float r_min, r_max;     /* metres */
    int32_t n_planes;       /* 0..2 half planes per view */
    int32_t flags;          /* GIE_GROUND_VIEW_* */
    int32_t reserved[4];    /* 0 */
} gie_ground_view_param;
int gie_ground_view_gain(gie_mapper *h, const float *xy, const int32_t *normals, int n, const gie_ground_view_param *p, gie_view_score *out);
int gie_ground_view_gain_dev(gie_mapper *h, const float *d_xy, const int32_t *d_normals, int n, const gie_ground_view_param *p, gie_view_score *d_out);
int gie_ground_view_mask(gie_mapper *h, const float *xy, const int32_t *normals, const gie_ground_view_param *p, uint8_t *mask, gie_view_score *score);
int gie_ground_view_mask_dev(gie_mapper *h, const float *d_xy, const int32_t *d_normals, const gie_ground_view_param *p, uint8_t *d_mask, gie_view_score *d_score);

/* ---- ground rollouts: n candidate trajectories of T poses each, scored on the ground costmap in one call — the local half of a ground
 * robot's navigation, beside the global half of "ground navigation function" and "ground line of sight".  A sampling-based local
 * planner (DWA, trajectory rollout, MPPI) draws a few thousand short trajectories from the robot's pose, drops those that collide and
 * scores the rest by how close they pass to obstacles and how far they get down the navigation function.  One call returns ONE record
 * per trajectory; chaining gie_ground_segments_dev, gie_ground_query_dev and gie_ground_nf1_query_dev over the n * T poses instead
 * returns n * T records of 24 + 16 + 4 bytes for the host to reduce, and cannot give the per-cell cost.  No counterpart in the
 * reference's code.
 *
 * Every call refers to the ground field that is valid where the call is enqueued (the rule of "ground line of sight"): there is no
 * prepare call and no kept result, a later gie_ground_compute* makes later calls see the new field, a map update changes nothing.
 * With GIE_GROUND_ROLLOUT_NF1 the call also reads the ground navigation function of that field; it writes neither.  Everything is
 * an integer: a result depends on no schedule.
 *  poses         xy holds pose k of trajectory i at xy[2 * (i * T + k)], two floats, metres, world frame.
 *  c_k           the cell of pose k, gie_ground_query's mapping: gie_pos2coord(xy, w) - pvt per axis.  A pose that is not finite (NaN,
 *                +-inf), that no int32 coordinate holds, or that lies outside the field's rectangle has NO cell.
 *  blocked(c)    the rule of "ground line of sight" with clearance_sq and GIE_GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE.
 *  reached       pose k is REACHED iff every pose 0 .. k has a cell, c_0 is not blocked, and no cell of L2(c_{j-1}, c_j) is blocked
 *                for 1 <= j <= k; L2 is the cell line of "ground line of sight", tie rule included: a wall one cell thick between
 *                two consecutive samples is found.
 *  poses         m, the number of reached poses, 0 .. T.
 *  end           0 when m == T; otherwise 2 when pose m has no cell; otherwise 1: leg m is blocked, and hit is its first blocked
 *                cell in walking order from c_{m-1} (c_0 itself when m == 0), in GLOBAL cell coordinates (local + pivot).  A NaN
 *                tail is the way to pass rollouts shorter than T: they end with 2.
 *  the prefix's cells  c_0, then for j = 1 .. m - 1 the cells of L2(c_{j-1}, c_j) after its first.  Two equal consecutive cells add
 *                nothing; a cell that two different legs cross counts twice.  cells is their number, min_dist_sq the minimum of the
 *                field's dist_sq over them (-1 on a field without an obstacle column) and cost the sum of
 *                max(0, inflate_sq - dist_sq) over them, a dist_sq of -1 costing 0: at most 2^22 per cell, a 64-bit sum.  With
 *                m == 0 all three are 0.
 *  NF1           with GIE_GROUND_ROLLOUT_NF1, the values gie_ground_nf1_query returns at c_0 .. c_{m-1}: nf1_end is the one at
 *                c_{m-1} (-1 when that cell is unreachable or m == 0), nf1_min the least value >= 0 among them (-1 when there is
 *                none) and nf1_min_at the FIRST pose that has it (-1).  Without the flag all three are -2.
 * GIE_ERR_INVALID, nothing written: a NULL handle; a tiled mapper; no ground field yet; a NULL param; clearance_sq < 0; inflate_sq
 *  outside 0 .. 1 << 22; an unknown flag; non-zero reserved; GIE_GROUND_ROLLOUT_NF1 without a valid ground navigation function (a
 *  gie_ground_compute* invalidates it); n < 0; T outside 1 .. GIE_GROUND_ROLLOUT_MAX_POSES; n > 0 with a NULL buffer; in the host form,
 *  n * T * 8 bytes beyond size_t.  n == 0 is valid and launches nothing; n has no upper limit.
 * The host form stages through the two scratch slots of the host forms and synchronises.  The _dev form takes DEVICE buffers and is
 *  enqueued on the mapper's stream (gie_get_stream) with no host wait, no read-back and no grid barrier.
 * Memory: nothing of its own: the blocked bit plane is the one of "ground line of sight", allocated by the first call of either.
 * Cost: a call is two launches: the blocked plane, as there, and the rollouts: a wave per trajectory, a lane per pose in chunks of 64,
 *  each lane walking the leg that ends at its pose; the chunk with the first blocked leg is the last.
 * gie_profile_read: counted under "ground_query". */
#define GIE_GROUND_ROLLOUT_UNKNOWN_TRAVERSABLE 1   /* as GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE */
#define GIE_GROUND_ROLLOUT_NF1                 2   /* gather the ground NF1 at the poses; needs a valid ground NF1 */
#define GIE_GROUND_ROLLOUT_MAX_POSES 4096
typedef struct gie_ground_rollout_param {   /* 32 bytes */
    int32_t clearance_sq;   /* blocked = ground line of sight's rule, squared cells, >= 0 */
    int32_t inflate_sq;     /* 0 .. 1 << 22: a cell costs max(0, inflate_sq - dist_sq); 0 = no cost */
    int32_t flags;          /* GIE_GROUND_ROLLOUT_* */
    int32_t reserved[5];    /* must be 0 */
} gie_ground_rollout_param;
typedef struct gie_ground_rollout {         /* 48 bytes */
    int32_t end;            /* 0 complete, 1 blocked, 2 left: pose `poses` has no cell (outside the field or not finite) */
    int32_t poses;          /* m: the poses of the clear prefix, 0 .. T */
    int32_t hit[2];         /* end == 1: the first blocked cell, in the field's global cell coordinates; otherwise 0, 0 */
    int32_t cells;          /* cells of the prefix's polyline, every joint once; 0 when m == 0 */
    int32_t min_dist_sq;    /* over those cells; -1 when the field has no obstacle column; 0 when m == 0 */
    int64_t cost;           /* over those cells: sum of max(0, inflate_sq - dist_sq); a dist_sq of -1 costs 0 */
    int32_t nf1_end;        /* ground NF1 at pose m - 1 (-1 unreachable or m == 0); -2 without GIE_GROUND_ROLLOUT_NF1 */
    int32_t nf1_min;        /* the least value >= 0 at the prefix's poses, -1 if there is none; -2 without the flag */
    int32_t nf1_min_at;     /* the first pose that has it, -1; -2 without the flag */
    int32_t reserved;       /* 0 */
} gie_ground_rollout;
int gie_ground_rollouts(gie_mapper *h, const float *xy, int n, int T, const gie_ground_rollout_param *p, gie_ground_rollout *out);
int gie_ground_rollouts_dev(gie_mapper *h, const float *d_xy, int n, int T, const gie_ground_rollout_param *p, gie_ground_rollout *d_out);

/* ---- ground footprints: the poses of n candidate trajectories tested as ORIENTED RECTANGLES of cells on the ground costmap — the
 * step of a costmap-based local planner (DWA, trajectory rollout, MPPI with a footprint critic) between "sampled a trajectory" and
 * "scored it".  Every other rule of the ground stack takes the robot for a disc and tests one cell against clearance_sq; a
 * 1.0 m x 0.6 m base does not enter a 0.8 m corridor at its circumscribed radius, and its corners pass through walls at its
 * inscribed one.  Here a pose has a heading, the reference point may lie anywhere on the long axis (front and back extents), and
 * one call returns ONE record per trajectory.  No counterpart in the reference's code.
 *
 * Every call refers to the ground field that is valid where the call is enqueued (the rule of "ground line of sight"): there is no
 * prepare call and no kept result, a later gie_ground_compute* makes later calls see the new field, a map update changes nothing.
 * Neither the field nor the ground navigation function is written.  Everything is an integer and exact: a result depends on no
 * schedule.  The poses are tested one by one, not the area swept between them: sample at a cell or less.
 *  poses         xy and heading are laid out as the rollouts' xy: pose k of trajectory i is at xy[2 * (i * T + k)] (two floats,
 *                metres, world frame) and heading[2 * (i * T + k)] (two int32, hx, hy: a direction vector of any length).
 *  placement     a pose has NO placement when its xy has no cell by the rollouts' rule (not finite, beyond int32, outside the
 *                field's rectangle), when its heading is (0, 0), or when a heading component is beyond +-32767.  The same in the
 *                host and _dev forms: neither scans the arrays on the host.  A NaN or zero-heading tail is the way to pass
 *                trajectories shorter than T.
 *  footprint     with c the pose's cell and, for any cell v inside the rectangle or not, d = v - c, n2 = hx^2 + hy^2,
 *                a = dx hx + dy hy, b = dx hy - dy hx: v is a FOOTPRINT cell iff, in int64 arithmetic, b^2 <= side_sq n2 and
 *                a^2 <= (a >= 0 ? front_sq : back_sq) n2.  front_sq, back_sq, side_sq are squared cells in
 *                0 .. GIE_GROUND_FOOTPRINT_MAX_SQ (no product reaches 2^63).  c is always a footprint cell; every footprint cell has
 *                |d|^2 <= max(front_sq, back_sq) + side_sq (a^2 + b^2 = |d|^2 n2); every row of the footprint is one interval of
 *                x.  A positive integer multiple of the heading gives the same set; with all three extents 0 it is c alone.
 *  blocked       a footprint cell inside the rectangle: the rule of "ground line of sight" with clearance_sq and
 *                GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE — clearance_sq pads the rectangle by a disc.  A footprint cell outside
 *                the rectangle is an UNKNOWN column without a dist_sq: blocked without the flag, not blocked with it.
 *  poses         m, the number of leading poses that have a placement and no blocked footprint cell, 0 .. T.
 *  end           0 when m == T; otherwise 2 when pose m has no placement; otherwise 1: hit is the blocked footprint cell of pose m
 *                that is least in (y, x) lexicographic order of signed local coordinates, reported in GLOBAL cell coordinates
 *                (local + pivot; it may lie outside the rectangle), and hit_cells the number of blocked footprint cells of pose
 *                m.  In the other cases hit is 0, 0 and hit_cells 0.
 *  margin        with GIE_GROUND_FOOTPRINT_MARGIN, min_dist_sq is the minimum of the field's dist_sq over the footprint cells of
 *                poses 0 .. m - 1 that lie inside the rectangle (-1 on a field without an obstacle column) and min_at the FIRST
 *                pose that attains it: the footprint critic's score.  With m == 0 they are 0 and -1.  Without the flag both are
 *                -2 and dist_sq is not read.
 *  mask          gie_ground_footprint_mask*: ONE pose (T = 1); mask is X * Y bytes, x fastest: 0 not a footprint cell, 1 a
 *                footprint cell that is not blocked, 2 a blocked footprint cell.  Footprint cells outside the rectangle have no
 *                byte but count in the record, which is the T = 1 record of that pose.  A pose without a placement gives an all-0
 *                mask and end = 2.  rec may be NULL.
 * GIE_ERR_INVALID, nothing written: a NULL handle or param; a tiled mapper; no ground field yet; an extent outside its range;
 *  clearance_sq < 0; an unknown flag; non-zero reserved; n < 0; T outside 1 .. GIE_GROUND_ROLLOUT_MAX_POSES; n > 0 with a NULL xy,
 *  heading or out; a NULL mask; in the host form, n * T * 16 bytes beyond size_t.  n == 0 is valid and launches nothing; n has no
 *  upper limit.
 * The host forms stage through the two scratch slots of the host forms (the poses and the headings share the first) and synchronise.
 *  The _dev forms take DEVICE buffers and are enqueued on the mapper's stream (gie_get_stream) with no host wait, no read-back and
 *  no grid barrier.
 * Memory: nothing of its own: the blocked bit plane is the one of "ground line of sight", allocated by the first call of either.
 * Cost: a call is two launches: the blocked plane, as there, and the footprints: a wave per trajectory, the poses in order, a lane
 *  per footprint row testing the masked 64-bit words of its interval; the first pose that ends the prefix is the last one looked
 *  at.  The mask forms zero the mask with a memset in front of the two launches.
 * gie_profile_read: counted under "ground_query". */
#define GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE 1   /* as GIE_GROUND_LOS_UNKNOWN_TRAVERSABLE; footprint cells outside the rectangle do not block */
#define GIE_GROUND_FOOTPRINT_MARGIN              2   /* min_dist_sq and min_at over the clear prefix's footprints */
#define GIE_GROUND_FOOTPRINT_MAX_SQ (1 << 16)
typedef struct gie_ground_footprint_param {  /* 32 bytes */
    int32_t front_sq;       /* squared cells ahead of the reference point along the heading, 0 .. GIE_GROUND_FOOTPRINT_MAX_SQ */
    int32_t back_sq;        /* behind it */
    int32_t side_sq;        /* to either side: the half width */
    int32_t clearance_sq;   /* blocked = ground line of sight's rule, squared cells, >= 0 */
    int32_t flags;          /* GIE_GROUND_FOOTPRINT_* */
    int32_t reserved[3];    /* must be 0 */
} gie_ground_footprint_param;
typedef struct gie_ground_footprint {        /* 32 bytes */
    int32_t end;            /* 0 complete, 1 blocked, 2 pose `poses` has no placement */
    int32_t poses;          /* m: the poses of the clear prefix, 0 .. T */
    int32_t hit[2];         /* end == 1: the least blocked footprint cell of pose m in (y, x) order, global cell coordinates; otherwise 0, 0 */
    int32_t hit_cells;      /* end == 1: the blocked footprint cells of pose m; otherwise 0 */
    int32_t min_dist_sq;    /* over the inside footprint cells of poses 0 .. m - 1; -1 no obstacle column; 0 when m == 0; -2 without the flag */
    int32_t min_at;         /* the first pose that attains it; -1 when m == 0; -2 without the flag */
    int32_t reserved;       /* 0 */
} gie_ground_footprint;
int gie_ground_footprints(gie_mapper *h, const float *xy, const int32_t *heading, int n, int T, const gie_ground_footprint_param *p, gie_ground_footprint *out);
int gie_ground_footprints_dev(gie_mapper *h, const float *d_xy, const int32_t *d_heading, int n, int T, const gie_ground_footprint_param *p, gie_ground_footprint *d_out);
int gie_ground_footprint_mask(gie_mapper *h, const float *xy, const int32_t *heading, const gie_ground_footprint_param *p, uint8_t *mask, gie_ground_footprint *rec);
int gie_ground_footprint_mask_dev(gie_mapper *h, const float *d_xy, const int32_t *d_heading, const gie_ground_footprint_param *p, uint8_t *d_mask, gie_ground_footprint *d_rec);

/* ---- ground pose navigation function: NF1 over (cell, heading) STATES of an oriented rectangle on the ground costmap — the global
 * planner of a base that is no disc.  "ground navigation function", "ground cost matrix" and the host layer's ground_plan() know
 * one number, clearance_sq: at the circumscribed radius a 1.0 m x 0.6 m base finds no route through a door it fits through
 * lengthwise, at the inscribed one it is sent round a corner it cannot turn in.  This section is the navigation function of the
 * configuration space "ground footprints" defines: the route length from every pose to the goal, and a descent a rectangular
 * robot can follow pose by pose.  No counterpart in the reference's code.
 *
 * Everything refers to the ground field that is valid where gie_ground_pose_nf1_compute* is enqueued (the rule of "ground
 * navigation function").  Integers only and exact: a result depends on no schedule.
 *  states        (c, k): c a cell of the field's X x Y rectangle, k in 0 .. GIE_GROUND_POSE_HEADINGS - 1 a heading, counter-clockwise
 *                from +x: d_0 = (1, 0), d_1 = (1, 1), d_2 = (0, 1), d_3 = (-1, 1), d_4 = (-1, 0), d_5 = (-1, -1), d_6 = (0, -1),
 *                d_7 = (1, -1).
 *  free          (c, k) is free iff the footprint of "ground footprints" placed at c with heading d_k (front_sq, back_sq, side_sq,
 *                clearance_sq, GIE_GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE with the meaning of GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE)
 *                has no blocked footprint cell; that section's predicate, blocked rule and treatment of footprint cells outside
 *                the rectangle apply word for word: gie_ground_footprints with T = 1 returns end == 1 for a pose in cell c with
 *                heading d_k iff (c, k) is not free.  With all three extents 0 a state is free iff its cell is not blocked and
 *                the eight layers are equal.  The extents are in 0 .. GIE_GROUND_POSE_MAX_SQ (64 cells: every footprint cell within
 *                90 cells of c, a footprint row at most 181 cells).
 *  moves         from (c, k): F to (c + d_k, k); B to (c - d_k, k), only with GIE_GROUND_POSE_NF1_REVERSE; L to (c, (k + 1) & 7);
 *                R to (c, (k + 7) & 7).  A move is admissible when its target lies inside the rectangle and is free.  Only the
 *                two states are tested, not the area swept between them (as "ground footprints" tests poses one by one).  Every
 *                move costs 1; a diagonal F covers more ground than an axial one for the same cost.
 *  sources       the free states among: for goal i, the cell of goal_xy[2i ..] by gie_ground_query's mapping (a goal without a
 *                cell is ignored: a NaN tail passes) with heading goal_k[i] — 0 .. 7 that one state, -1 all eight, any other value
 *                the goal is ignored; goal_k == NULL means -1 for every goal — and, with GIE_GROUND_POSE_NF1_FROM_FRONTIERS, every
 *                (c, k) whose cell is FNT.  n == 0 is valid.
 *  pnf1          pnf1(c, k) = the least number of admissible moves from (c, k) to a source: 0 on sources, -1 where there is none
 *                (states that are not free included).  8 * X * Y int32, k slowest: (k * Y + y) * X + x.  Without REVERSE the
 *                moves are not symmetric: the propagation expands predecessors.
 *  cspace        X * Y bytes, x fastest: bit k set iff (c, k) is not free.
 *  counts        two int32: the distinct source states, the free states.  May be NULL.
 *  query         for each of n (xy, k): k in 0 .. 7 pnf1 at that state; k == -1 the least value >= 0 over the eight headings, or
 *                -1; no cell, or any other k, -1.  k == NULL means -1 for every point.
 *  path          for each of n starts (xy, k): len = 0 for a start without a cell, a k outside -1 .. 7 or a value < 0; k == -1 (and
 *                start_k == NULL) picks the lowest k among those with the least value >= 0.  v_0 is the start state, v_{i+1} the
 *                first among F, B, L, R of v_i whose value is pnf1(v_i) - 1 (B only if the field was computed with REVERSE).
 *                len = pnf1 + 1, also when that exceeds max_len.  path_xyk holds max_len triples per start: GLOBAL x, y and k;
 *                exactly min(len, max_len) are written, the rest is left as it was.
 * Lifetime: the field is kept until the next gie_ground_pose_nf1_compute*; a gie_ground_compute* invalidates it, as it does the
 *  ground navigation function (readers, query and path then return GIE_ERR_INVALID); a map update changes nothing.  The ground
 *  navigation function and this field neither read nor invalidate each other; the ground field and the ground navigation function
 *  are byte-identical before and after every call of this section.
 * GIE_ERR_INVALID, nothing written: a NULL handle or param; a tiled mapper; no ground field yet; an extent outside its range;
 *  clearance_sq < 0; an unknown flag; non-zero reserved; n < 0; n > 0 with a NULL xy or output; max_len < 1; both outputs of the
 *  reader NULL; a read, query or path before a compute or after an invalidation.
 * The host forms stage through the two scratch slots of the host forms and synchronise.  The _dev forms take DEVICE buffers and are
 *  enqueued on the mapper's stream (gie_get_stream) with no host wait, no read-back and no grid barrier; the _dev goal array is
 *  gie_read_ground_frontier_clusters_dev's goal array, taken with its NaN tail as it is.
 * Memory: allocated at the first compute, freed by gie_destroy: 36 bytes per cell (the field 32, four bit planes of eight
 *  layers 4) and four control words; the blocked plane is the one of "ground line of sight".  A mapper that never calls the section
 *  allocates and launches nothing.
 * Cost: a compute is the blocked plane, the C-space (bit-parallel: shifted ORs of blocked words), the sources, and ONE workgroup
 *  that runs the levels with one workgroup barrier each, in LDS up to 768 words per layer, on global planes beyond.
 * gie_profile_read: the section adds no name; every call is counted under "ground_nf1", one entry per call. */
#define GIE_GROUND_POSE_NF1_UNKNOWN_TRAVERSABLE 1   /* as GIE_GROUND_FOOTPRINT_UNKNOWN_TRAVERSABLE */
#define GIE_GROUND_POSE_NF1_FROM_FRONTIERS      2   /* every state of an FNT cell is a source candidate */
#define GIE_GROUND_POSE_NF1_REVERSE             4   /* the move B */
#define GIE_GROUND_POSE_HEADINGS 8
#define GIE_GROUND_POSE_MAX_SQ (1 << 12)
typedef struct gie_ground_pose_nf1_param {   /* 32 bytes */
    int32_t front_sq;       /* squared cells ahead of the reference point along the heading, 0 .. GIE_GROUND_POSE_MAX_SQ */
    int32_t back_sq;        /* behind it */
    int32_t side_sq;        /* to either side: the half width */
    int32_t clearance_sq;   /* blocked = ground line of sight's rule, squared cells, >= 0 */
    int32_t flags;          /* GIE_GROUND_POSE_NF1_* */
    int32_t reserved[3];    /* must be 0 */
} gie_ground_pose_nf1_param;
int gie_ground_pose_nf1_compute(gie_mapper *h, const float *goal_xy, const int32_t *goal_k, int n, const gie_ground_pose_nf1_param *p, int32_t *counts);
int gie_ground_pose_nf1_compute_dev(gie_mapper *h, const float *d_goal_xy, const int32_t *d_goal_k, int n, const gie_ground_pose_nf1_param *p, int32_t *d_counts);
int gie_read_ground_pose_nf1(gie_mapper *h, int32_t *pnf1, uint8_t *cspace);
int gie_read_ground_pose_nf1_dev(gie_mapper *h, int32_t *d_pnf1, uint8_t *d_cspace);
int gie_ground_pose_nf1_query(gie_mapper *h, const float *xy, const int32_t *k, int n, int32_t *steps);
int gie_ground_pose_nf1_query_dev(gie_mapper *h, const float *d_xy, const int32_t *d_k, int n, int32_t *d_steps);
int gie_ground_pose_nf1_path(gie_mapper *h, const float *start_xy, const int32_t *start_k, int n, int max_len, int32_t *path_xyk, int32_t *len);
int gie_ground_pose_nf1_path_dev(gie_mapper *h, const float *d_start_xy, const int32_t *d_start_k, int n, int max_len, int32_t *d_path_xyk, int32_t *d_len);

/* ---- ground signed distance: the ground costmap continued into the obstacles, a distance and a gradient at continuous points and
 * the clearance of whole trajectories — what the optimising planners (TEB, CHOMP, MPC, elastic bands) take where the search planner
 * takes "ground navigation function" and the sampling one "ground rollouts".  gie_ground_query returns the integer dist_sq of the
 * one cell a point falls into: a step function without a slope, and 0 on every obstacle column, so a pose inside an obstacle (a
 * wall moved onto the robot by a map update; any unknown region with GIE_GROUND_UNKNOWN_BLOCKS) is not pushed out.  This is
 * "signed distance field" in the plane, on the ground field; that section's own field is of no use to a ground robot (the floor is
 * one voxel away everywhere).  No counterpart in the reference's code.
 *
 * Everything refers to the ground field that is valid where the call is enqueued (the rule of "ground line of sight"): its pivot,
 * its rectangle X x Y, its obstacle columns — OCCUPIED, and UNKNOWN too when the field was computed with GIE_GROUND_UNKNOWN_BLOCKS.
 *  inside_dist_sq(x, y)  0 on a column that is not an obstacle column; on an obstacle column the exact squared Euclidean distance,
 *                     in cells and as an integer, to the nearest non-obstacle column OF THE RECTANGLE; -1 when the rectangle holds
 *                     no non-obstacle column.
 *  gsdf(x, y)         cell units, like gie_seendist.d:
 *                       inside_dist_sq <= 1:  the `d` gie_read_costmap_ground writes for the cell, bit for bit:
 *                                             sqrtf((float)dist_sq), or (float)max_loc_dist_sq on a field without an obstacle column;
 *                       inside_dist_sq >  1:  1.0f - sqrtf((float)inside_dist_sq);
 *                       inside_dist_sq == -1: -(float)max_loc_dist_sq.
 *                     "signed distance field"'s convention: the surface layer of an obstacle stays at 0, deeper columns go
 *                     negative.  The field differs from the ground costmap ONLY on obstacle columns all four of whose edge
 *                     neighbours inside the rectangle are obstacle columns.
 * Query at a point p (metres, world frame), "signed distance field"'s with the z axis removed, on the FIELD's pivot.  The order of
 * the float32 operations is part of the contract (the library is compiled without contraction into fused multiply-adds):
 *  u_k = p_k / w - (float)pvt_k    continuous local coordinate (cell centres at integers);
 *  axis with size_k >= 2:          inside iff 0 <= u_k <= size_k - 1; i0 = min((int)floorf(u_k), size_k - 2), t_k = u_k - (float)i0;
 *  axis with size_k == 1:          inside iff -0.5 <= u_k < 0.5; i0 = i1 = 0, t_k = 0; its gradient component is exactly 0;
 *  corners                         v0 = gsdf(i0x, i0y), v1 = gsdf(i1x, i0y), v2 = gsdf(i0x, i1y), v3 = gsdf(i1x, i1y);
 *  weights                         sx = 1 - tx, sy = 1 - ty;  c0 = v0 * sx + v1 * tx, c1 = v2 * sx + v3 * tx;
 *  dist    (c0 * sy + c1 * ty) * w: metres;
 *  grad    grad_x = (v1 - v0) * sy + (v3 - v2) * ty, grad_y = c1 - c0 (n x 2, x y per point): m/m;
 *  flags   bit 0 inside the rectangle, bit 1 all corners known (type != UNKNOWN), bit 2 some corner an obstacle column;
 *  outside the rectangle, NaN, +-inf: dist = NaN, grad = 0, 0, flags = 0.
 * Rollouts: n trajectories of T points, laid out as "ground rollouts" lays out its poses (point k of trajectory i at
 *  xy[2 * (i * T + k)]), 1 <= T <= GIE_GROUND_ROLLOUT_MAX_POSES; a NaN tail passes shorter trajectories.  One record per trajectory,
 *  every field a pure function of the per-point query results: minima, first indices and counts, no sum of floats — no result
 *  depends on a schedule.  The optional per-point outputs dist (n * T) and grad (2 * n * T) hold exactly what gie_ground_query_sdf
 *  writes for every point, in the prefix or behind it.
 * Cache: inside_dist_sq belongs to ONE ground field: it is computed on the device at the first call of this section after a
 *  gie_ground_compute* and kept until the next one; a map update changes nothing, as it changes nothing of the ground field.  The
 *  device counts the interior obstacle columns (those whose four edge neighbours are obstacle columns, outside the rectangle
 *  counting as one) from the bit rows; with none the exact transform returns at once and 0 / 1 is read off the bit rows.  No call
 *  waits on the host for that.
 * Memory: 4 bytes per cell and one int32, allocated at the first call of the section, freed by gie_destroy.  A mapper that never
 *  calls the section allocates and launches nothing.  The section writes nothing of the map, of the ground field or of any other
 *  stage's field.
 * Arguments: sdf / inside_dist_sq are X * Y values each (x fastest), either may be NULL, not both; dist (n), grad (2n) and flags (n)
 *  may each be NULL, not all three; the rollouts' dist and grad may each be NULL; n == 0 is valid and launches nothing.
 * GIE_ERR_INVALID, nothing written: a NULL handle; a tiled mapper; no ground field yet; all outputs NULL; n < 0; n > 0 with a NULL
 *  xy; for the rollouts a NULL param, n > 0 with a NULL record buffer, a margin that is negative or not finite, non-zero flags or
 *  reserved, T outside 1 .. GIE_GROUND_ROLLOUT_MAX_POSES and, in the host form, n * T * 8 bytes beyond size_t.
 * The host forms stage through the two scratch slots of the host forms and synchronise.  The _dev forms take DEVICE buffers and are
 *  enqueued on the mapper's stream (gie_get_stream) with no host wait, no read-back and no grid barrier.
 * Cost: the inside pass is a memset of the count and two launches (the count; one wave per x for the transform, as the ground
 *  field's own); a read, a query and a rollout call are one launch each behind it: a lane per cell or point, a wave per trajectory
 *  with a lane per point in chunks of 64.
 * gie_profile_read: the section adds no name: the inside pass and gie_read_ground_sdf* are counted under "ground", the queries and
 *  the rollouts under "ground_query" (a call that runs the inside pass first adds one entry to each). */
typedef struct gie_ground_sdf_rollout_param {   /* 32 bytes */
    float   margin;         /* metres, finite, >= 0: a point is BELOW with dist < margin */
    int32_t flags;          /* must be 0 */
    int32_t reserved[6];    /* must be 0 */
} gie_ground_sdf_rollout_param;
typedef struct gie_ground_sdf_rollout {         /* 32 bytes */
    int32_t points;         /* m: the leading points whose query has flag bit 0; the first point without it ends the prefix */
    int32_t argmin;         /* the FIRST k < m with the least dist; -1 when m == 0 */
    float   min_dist;       /* that dist, metres; NaN when m == 0 */
    float   grad[2];        /* the query's gradient at argmin; 0, 0 when m == 0 */
    int32_t first_below;    /* the first k < m with dist < margin; -1 */
    int32_t n_below;        /* how many k < m have dist < margin */
    int32_t first_in;       /* the first k < m with dist <= 0 (on or inside an obstacle); -1 */
} gie_ground_sdf_rollout;
int gie_read_ground_sdf(gie_mapper *h, float *sdf, int32_t *inside_dist_sq);
int gie_read_ground_sdf_dev(gie_mapper *h, float *d_sdf, int32_t *d_inside_dist_sq);
int gie_ground_query_sdf(gie_mapper *h, const float *xy, int n, float *dist, float *grad, uint8_t *flags);
int gie_ground_query_sdf_dev(gie_mapper *h, const float *d_xy, int n, float *d_dist, float *d_grad, uint8_t *d_flags);
int gie_ground_sdf_rollouts(gie_mapper *h, const float *xy, int n, int T, const gie_ground_sdf_rollout_param *p, gie_ground_sdf_rollout *out,
                            float *dist, float *grad);
int gie_ground_sdf_rollouts_dev(gie_mapper *h, const float *d_xy, int n, int T, const gie_ground_sdf_rollout_param *p, gie_ground_sdf_rollout *d_out,
                                float *d_dist, float *d_grad);

/* ---- goal-to-goal cost matrix: the path lengths among up to 64 points (the robot and the goals of the frontier clusters, say), the
 * input of every tour-based explorer — in which order to visit the clusters.  n fields of gie_nf1_compute would give the same
 * numbers with n persistent launches and n whole fields; here ONE level-synchronous pass advances all searches, a 64-bit mask per
 * voxel.  No counterpart in the reference's code.
 *
 * Everything is over the local volume at the point of the mapper's stream where gie_costmat_compute* is enqueued; type(v) and
 * edt(v) are exactly what gie_read_local would return there.
 *  traversable(v)  NF1's rule: type(v) is FREE or FNT (or UNKNOWN, with GIE_NF1_UNKNOWN_TRAVERSABLE) and edt(v) >= clearance (a
 *                  float comparison; clearance in voxel units).  GIE_NF1_FROM_FRONTIERS has no meaning here: GIE_ERR_INVALID.
 *  voxel(i)        of point i (metres, world frame), as NF1's goals: gie_pos2coord(p_k, w) - pvt_k.  The point is VALID when it is
 *                  finite, inside the volume and its voxel traversable.  valid[i] = 1 or 0 (valid may be NULL).
 *  cost            n x n int32, row-major.  cost[i][j] = the number of steps of the shortest 6-connected path from voxel(i) to
 *                  voxel(j) whose every voxel is traversable and inside the volume; 0 when the voxels coincide (i = j included);
 *                  -1 when either point is invalid or there is no such path.  The matrix is symmetric, the rows of invalid points
 *                  are all -1, two points on one voxel have identical rows.  By definition cost[i][j] is the value at voxel(i) of
 *                  the field gie_nf1_compute gives for the single goal j with the same clearance and flags.
 * Arguments: 0 <= n <= GIE_COSTMAT_MAX_POINTS, otherwise GIE_ERR_INVALID; n == 0 is valid and writes nothing.  A NULL p, a NULL
 *  xyz or cost with n > 0, a clearance that is negative or not finite, an unknown flag and a tiled mapper (as NF1: the searches
 *  would stop at the tile's faces) get GIE_ERR_INVALID.
 * The host form synchronises.  The _dev form takes DEVICE buffers and is enqueued on the mapper's stream without a host wait; the
 *  host needs neither the number of valid points nor the number of levels.  The goal array gie_read_frontier_clusters_dev writes
 *  (NaN in its unused entries) can stand behind a robot position in one buffer and be handed over as it is: max_clusters + 1
 *  points, the NaN ones invalid.
 * The result is complete when the call's work is done; nothing is kept for later readers.
 * Propagation: one persistent launch of gie_config.wave_workgroups workgroups with a grid barrier per BFS level, as NF1's, and
 *  like it a member of the device's chain of grid-barrier launches.  Level k computes seen_{k+1}(v) = seen_k(v) | the seen_k of
 *  the six neighbours from level k's masks only, on the tiles (64 x 8 x 8 voxels) in which something changed in level k - 1 and
 *  their face neighbours.  It ends when a level changes nothing, or earlier once every valid point's voxel holds the mask of all
 *  valid points; the matrix is the same either way.  The number of levels is the largest finite distance from a valid point to any
 *  voxel it reaches (with the early end: the largest entry of the matrix, when all valid points are connected).
 * If a grid barrier times out (the workgroups were kept off the device by another process), the next sync reports
 *  GIE_ERR_TIMEOUT through the error word the map update uses, with a message that says the matrix is incomplete (entries -1 that
 *  should be finite); the map itself is not affected.
 * Memory: scratch allocated at the first call (gie_dalloc, freed by gie_destroy): two planes of one 64-bit mask per voxel (16 bytes
 *  per voxel), one bit plane with rows padded to 64-bit words (0.125 bytes per voxel when X is a multiple of 64) and 12 bytes per
 *  tile of 64 x 8 x 8 voxels: 16.13 bytes per voxel in all, 2.2 GB at 512^3.  NF1's field and the map update do not read it. */
#define GIE_COSTMAT_MAX_POINTS 64
int gie_costmat_compute(gie_mapper *h, const float *xyz, int n, const gie_nf1_param *p, int32_t *cost, uint8_t *valid);
int gie_costmat_compute_dev(gie_mapper *h, const float *d_xyz, int n, const gie_nf1_param *p, int32_t *d_cost, uint8_t *d_valid);

/* ---- changed-block streaming: the CPU mirror the reference keeps for RViz and CPU planners.
 * GlbHashMap::streamPipeline / streamD2H / getUpdatedAddr (glb_hash_map.cu:209-247,
 * unify_helper.cuh:11-32), fed by the stream_VB_keys_D appends of the fuse / wave / commit kernels
 * (unify_helper.cuh:103-110,184-191,510-520; wave_core.cuh:129-134), switched by
 * display_glb_edt / display_glb_ogm (volumetric_mapper.cpp:182,196-198).
 * gie_stream_enable(1) makes the update kernels flag every block in which a voxel's type,
 * distance or closest obstacle changes (off by default: README.md:154).  gie_stream_changed
 * hands over the flagged blocks — key (block coordinate, 3 ints) + GIE_BLOCK_VOXELS voxels in the
 * reference's in-block order get_voxID_in_VB = (x&7)*64 + (y&7)*8 + (z&7)
 * (voxmap_utils.cuh:104-109) — and clears their flags.  *n_changed = flagged blocks before the
 * call; at most max_blocks are delivered (the rest stay flagged), in unspecified order; NULL
 * keys/blocks only counts.  One gather kernel + one batched copy per chunk instead of the
 * reference's 20 KB memcpy per block.
 * A delivered block holds what gie_query_global returns for its voxels at the call, whenever the
 * call comes: flags stay set while the stream is off, and a block flagged in one update may be
 * drained after later ones — records that those updates left to the pair plane are stored before
 * the gather (a call that delivers nothing, or only counts, does not pay for that). */
#define GIE_BLOCK_VOXELS 512
/* (takes effect with the next gie_fuse: a map update runs in one order of kernels — the fused Mark + commit sweep, or the reference's
 * Mark ... commit with the flags — from its fuse to its merge) */
int gie_stream_enable(gie_mapper *h, int on);
int gie_stream_changed(gie_mapper *h, int32_t *keys, gie_voxel *blocks, int max_blocks, int32_t *n_changed);

/* ---- spatial tiling across GPUs (no counterpart in the reference, which is single-GPU; SURVEY
 * §8e).  A large volume is cut into tiles, one mapper per tile/GPU.  Per map update every tile runs
 * fuse, batch EDT and gie_merge_begin_tiled on its own volume, exports the one-voxel layer on each of
 * its faces, imports its neighbours' layers as "ghost" voxels just outside its own volume — the role
 * old out-of-volume voxels play in the reference, but refreshed every update — and finishes with
 * gie_merge_end.  Then rounds of export / exchange / import / gie_refine (obtainFrontiers' C seeds
 * restricted to the faces → wave C → commit) repeat until no tile changes.  Voxels of ANOTHER tile
 * are only ever read as ghosts: waves A / B (raise / lower outside) run outside the whole volume.
 * face = 2*axis + side (0:-x 1:+x 2:-y 3:+y 4:-z 5:+z); a layer is indexed b*A + a with (a,b) the
 * two remaining axes in x<y<z order. */
typedef struct gie_halo_voxel {
    int32_t dist_sq;
    int32_t coc[3];
    int8_t vox_type;
    uint8_t occ_val;   /* travels too: a ghost voxel that enters the tile next frame keeps its occupancy state */
    int8_t pad[2];
} gie_halo_voxel;
/* Tile placement: the local volume is centred `off` voxels away from the sensor position
 * (_pvt = round(pos/w) - size/2 + off); every tile of one robot shares the sensor pose and the
 * wave-range pivot.  `whole` = size of the union of all tiles (centred on the sensor like an
 * ordinary local volume): MarkLimitedObserve keeps an old distance only when its closest
 * obstacle lies outside the WHOLE volume — one inside another tile is re-derived from that
 * tile's current state through the halo exchange instead of being trusted.  Takes effect at the
 * next gie_set_pose; default off = 0, whole = local_size = the reference. */
int gie_set_tile(gie_mapper *h, const int32_t off[3], const int32_t whole[3]);
int gie_halo_count(gie_mapper *h, int face);
int gie_halo_export(gie_mapper *h, int face, gie_halo_voxel *out);
int gie_halo_import(gie_mapper *h, int face, const gie_halo_voxel *in);
/* same with DEVICE buffers (RCCL send/recv tensors), asynchronous on the mapper's stream */
int gie_halo_export_dev(gie_mapper *h, int face, gie_halo_voxel *d_out);
int gie_halo_import_dev(gie_mapper *h, int face, const gie_halo_voxel *d_in);
/* SPARSE face layers: only the KNOWN voxels of a layer, as (index in the layer, record) in no particular order.  An unknown ghost
 * changes nothing on import, so the two forms are interchangeable and may be mixed from round to round; a layer of a sparsely
 * observed face (a lidar's) is a few per cent of the dense one, a fully observed face (BASELINE config 5) gains nothing.  `out`
 * holds gie_halo_count(face) entries at most; the count travels with the payload (the _dev forms keep it on the device: the
 * import launches over the whole layer and looks at the first *d_count entries, so nothing waits for the host). */
typedef struct gie_halo_entry { int32_t index; gie_halo_voxel v; } gie_halo_entry;
int gie_halo_export_sparse(gie_mapper *h, int face, gie_halo_entry *out, int32_t *count);
int gie_halo_import_sparse(gie_mapper *h, int face, const gie_halo_entry *in, int32_t count);
int gie_halo_export_sparse_dev(gie_mapper *h, int face, gie_halo_entry *d_out, int32_t *d_count);
int gie_halo_import_sparse_dev(gie_mapper *h, int face, const gie_halo_entry *d_in, const int32_t *d_count);
/* returns the number of voxels seeded from ghost neighbours in *seeded (0 = nothing changed) */
/* Several faces in one call (NULL entry = face not exchanged): one launch per step for all of
 * them and one block allocation for all ghost layers. */
int gie_halo_export_all_dev(gie_mapper *h, gie_halo_voxel *const d_out[6]);
int gie_halo_import_all_dev(gie_mapper *h, const gie_halo_voxel *const d_in[6]);
int gie_refine(gie_mapper *h, int32_t *seeded);   /* seeded == NULL: enqueue only (no synchronisation) */
/* Exchange rounds "until no GPU changed"  WITHOUT the host in the loop.  A caller enqueues a fixed upper bound of
 * rounds per map update on the mapper's stream — export, transfer, import, gie_refine_dev — and all-reduces (max) the word
 * gie_refine_dev leaves over the ranks, on the same stream (RCCL), into a device word it hands to gie_round_gate before the
 * next round: while that word is 0 every kernel of a round (export, ghost-block allocation, import, refinement) returns at once.
 * gie_refine_dev = gie_refine(h, NULL) + *d_changed = voxels seeded from ghost neighbours by this round (0 when the gate kept
 * it from running).  gie_round_gate(h, NULL) opens the gate (the first round of an update always runs).  gie_round_end closes a
 * map update's rounds: opens the gate and counts the update as unconverged when *d_go (the all-reduced word of the LAST round;
 * NULL = not known) is still non-zero.  gie_round_stats synchronises: out = { rounds enqueued, rounds that ran, map updates,
 * map updates left unconverged } since gie_create.  A gate lasts until gie_round_end or the next gie_set_pose, whichever comes
 * first (a caller that leaves a round half way does not gate the next update).  No counterpart in the reference (single GPU). */
int gie_round_gate(gie_mapper *h, const int32_t *d_go);
int gie_refine_dev(gie_mapper *h, int32_t *d_changed);
int gie_round_end(gie_mapper *h, const int32_t *d_go);
int gie_round_stats(gie_mapper *h, int64_t out[4]);
/* The HIP stream all work of this mapper is enqueued on (a hipStream_t), so that a caller can order
 * its own device work — e.g. the RCCL transfers of the halo layers — with it instead of
 * synchronising the host.  NULL for implementations without streams. */
int gie_get_stream(gie_mapper *h, void **stream);

/* Per-kernel device time (the reference only has the two std::chrono spans of
 * volumetric_mapper.cpp:153,187-203).  When enabled, every kernel launch of the frame carries
 * start / stop HIP events on the mapper's stream (on its own dispatch packet: the time is the
 * kernel's execution, `launches` counts the brackets a kernel group was timed in);
 * gie_profile_read synchronises, returns the accumulated totals since the last read and resets
 * them.  Profiling is not free: a timed dispatch makes the next one wait for its completion
 * signal (about +0.1 ms per map update on an MI355X) — leave it off when measuring throughput. */
typedef struct gie_kernel_time {
    char name[24];
    float total_ms;
    int32_t launches;
} gie_kernel_time;
int gie_profile_enable(gie_mapper *h, int on);
int gie_profile_read(gie_mapper *h, gie_kernel_time *out, int max_entries);
/* local pivot _pvt (global coord of local voxel 0,0,0) of the current frame. */
int gie_get_pivot(gie_mapper *h, int32_t pvt[3]);

#ifdef __cplusplus
}
#endif
#endif /* GIE_H */
