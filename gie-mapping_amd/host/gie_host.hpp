/*
 * gie_host.hpp — ROS-free C++ host layer over the C-ABI (include/gie.h).
 *
 * Counterpart of what the reference keeps on the host around the GPU path:
 *   Parameters            include/parameters.h:16-139 (defaults, flt2GridsSq) + the cfg yaml keys
 *   Vlp16Adapter          Vlp16MapMaker::convertPyntCld, src/vlp16_map_maker.cpp:73-147
 *   PointCloudAdapter     PntcldMapMaker::pntcld_process, src/pntcld_map_maker.cpp:49-61
 *   ExtObstacles          Ext_Obs_Wrapper, src/kernel/pre_map/pre_map.cu:4-101, and the DBSCAN
 *                         clustering of VOLMAPNODE::clustring, src/volumetric_mapper.cpp:391-491
 *   CsvLog                csvfile, include/simple_logger.h:18-85
 *   GroundTruthCheck      Gnd_truth_checker::cmp_dist, include/gt_checker.h:30-80
 *   BlockMirror           hash_table_H_std / VB_values_H / VB_keys_H fed by streamPipeline,
 *                         src/kernel/par_wave/glb_hash_map.cu:209-247, README.md:163-170
 *   VolumetricMapper      VOLMAPNODE ctor + publishMap, src/volumetric_mapper.cpp:6-224, with
 *                         CostMap = msg/CostMap.msg
 *   DisplayClouds         the four point clouds of VOLMAPNODE::visualize, include/volumetric_mapper.h:181-357
 * The ROS transport (subscriptions, message_filters, tf broadcast, the RViz publishers) is not part of it.
 * Written from the behaviour described in those files; no reference code is reused (PCL's
 * KD-tree / MomentOfInertia are replaced by plain loops).
 */
#ifndef GIE_HOST_HPP
#define GIE_HOST_HPP

#include <array>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gie.h"

/* exploration_costs chains device-side calls and needs a device buffer of its own: it exists where this header is compiled with the
 * HIP runtime's headers at hand (hipcc, or any compiler with -DGIE_HOST_WITH_HIP and the include path); the rest needs none */
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__) || defined(GIE_HOST_WITH_HIP)
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>
#define GIE_HOST_HAS_HIP 1
#endif

namespace gie_host {

struct Vec3 { float x, y, z; };

/* ---------------------------------------------------------------- parameters */
struct Parameters {
    bool for_motion_planner = false;
    float robot_r = 0.4f;
    bool display_loc_edt = false, display_loc_ogm = false, display_glb_edt = true, display_glb_ogm = true;
    bool cpu_mirror = true;              /* no counterpart in the reference, which always mirrors: the global display flags switch the changed-block stream on and
                                          * visualize() reads the mirror.  false: the stream stays off (the map update runs its fused sweep) and visualize() takes the
                                          * global clouds from the device (gie_cloud_global); `mirror` stays empty */
    float ground_min_height = 0.f, ground_max_height = -1.f;   /* no counterpart in the reference: the band of world z (metres) a ground robot's body occupies, for ground_costmap();
                                                                 * "ground/min_height", "ground/max_height"; off while max < min (the default) */
    int ground_min_known = 1;            /* "ground/min_known": gie_ground_param.min_known */
    float ground_robot_radius = 0.f;     /* "ground/robot_radius" (metres): ground_plan() keeps ceil(radius / voxel_width) cells away from every obstacle column */
    float ground_footprint[3] = { -1.f, -1.f, -1.f };   /* "ground/footprint": front, back, half width (metres) of the robot's rectangle around its reference
                                                          * point, three numbers ("0.7 0.3 0.3" or "[0.7, 0.3, 0.3]"); unset (the default) while one is negative */
    int explore_min_fnt = 1;             /* "explore/min_fnt": global_frontier_blocks() takes the blocks with at least this many FNT voxels (1..512) */
    int explore_route_min_free = 1;      /* "explore/route_min_free": global_frontier_routes() takes a block as a node with at least this many passable voxels (1..512) */
    int explore_route_min_open = 1;      /* "explore/route_min_open": ... and joins two blocks across a face with at least this many open voxel pairs (1..64) */
    bool profile_loc_rms = false, profile_glb_rms = false;
    std::string log_name = "GIE_log.csv";
    std::string data_case = "ugv_corridor";
    int vis_interval = 1;
    int occupancy_threshold = 180;
    float vis_height = 1.0f, ugv_height = -1.0f;
    float voxel_width = 0.2f;
    float local_size_x = 10, local_size_y = 10, local_size_z = 3;
    float ogm_min_h = 0.2f, ogm_max_h = 10.0f;
    bool fast_mode = true;               /* code default, parameters.h:93 */
    float cutoff_dist = 6.0f;
    int max_bucket = 10000, max_block = 19997;
    int wave_workgroups = 0, place_tries = 0;   /* gie_config fields of the same name (no counterpart in the reference): "gpu/wave_workgroups", "gpu/place_tries" */
    bool is_ext_obsv_3D = false;
    std::vector<Vec3> obsbbx_ll{ { -3.6f, -3.2f, 0.2f } }, obsbbx_ur{ { 4.4f, 3.4f, 2.6f } };   /* the hard-coded fence */

    int flt2GridsSq(float rad) const { const int g = (int)std::ceil(rad / voxel_width); return g * g; }
    int cutoff_grids_sq() const { return flt2GridsSq(cutoff_dist); }
    int robot_r2_grids() const { return flt2GridsSq(robot_r); }

    /* cfg yaml: flat "key: value" lines with one level of nesting (ogm:, wave:, hash:) */
    void load_yaml(const std::string &path)
    {
        std::ifstream f(path);
        if (!f) throw std::runtime_error("cannot open " + path);
        std::string line, section;
        while (std::getline(f, line)) {
            const size_t hash = line.find('#');
            if (hash != std::string::npos) line.erase(hash);
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
            const bool nested = line[0] == ' ' || line[0] == '\t';
            const size_t colon = line.find(':');
            if (colon == std::string::npos) continue;
            auto trim = [](std::string s) { const size_t a = s.find_first_not_of(" \t\r\""), b = s.find_last_not_of(" \t\r\""); return a == std::string::npos ? std::string() : s.substr(a, b - a + 1); };
            const std::string key = trim(line.substr(0, colon)), val = trim(line.substr(colon + 1));
            if (val.empty()) { section = key; continue; }
            if (!nested) section.clear();
            set(section.empty() ? key : section + "/" + key, val);
        }
    }
    void set(const std::string &k, const std::string &v)
    {
        auto b = [&] { return v == "true" || v == "True" || v == "1"; };
        auto fl = [&] { return std::stof(v); };
        auto in = [&] { return std::stoi(v); };
        if (k == "for_motion_planner") for_motion_planner = b(); else if (k == "robot_r") robot_r = fl();
        else if (k == "display_loc_edt") display_loc_edt = b(); else if (k == "display_loc_ogm") display_loc_ogm = b();
        else if (k == "display_glb_edt") display_glb_edt = b(); else if (k == "display_glb_ogm") display_glb_ogm = b();
        else if (k == "cpu_mirror") cpu_mirror = b();
        else if (k == "profile_loc_rms") profile_loc_rms = b(); else if (k == "profile_glb_rms") profile_glb_rms = b();
        else if (k == "log_name") log_name = v; else if (k == "data_case") data_case = v;
        else if (k == "vis_interval") vis_interval = in(); else if (k == "occupancy_threshold") occupancy_threshold = in();
        else if (k == "vis_height") vis_height = fl(); else if (k == "ugv_height") ugv_height = fl();
        else if (k == "voxel_width") voxel_width = fl();
        else if (k == "local_size_x") local_size_x = fl(); else if (k == "local_size_y") local_size_y = fl(); else if (k == "local_size_z") local_size_z = fl();
        else if (k == "ogm/min_height") ogm_min_h = fl(); else if (k == "ogm/max_height") ogm_max_h = fl();
        else if (k == "ground/min_height") ground_min_height = fl(); else if (k == "ground/max_height") ground_max_height = fl();
        else if (k == "ground/min_known") ground_min_known = in();
        else if (k == "ground/robot_radius") ground_robot_radius = fl();
        else if (k == "explore/min_fnt") explore_min_fnt = in();
        else if (k == "explore/route_min_free") explore_route_min_free = in();
        else if (k == "explore/route_min_open") explore_route_min_open = in();
        else if (k == "ground/footprint") {
            std::string t = v;
            for (char &ch : t) if (ch == '[' || ch == ']' || ch == ',') ch = ' ';
            std::istringstream is(t);
            float f3[3];
            if (!(is >> f3[0] >> f3[1] >> f3[2])) throw std::invalid_argument("ground/footprint: three numbers (front, back, half width)");
            for (int i = 0; i < 3; i++) ground_footprint[i] = f3[i];
        }
        else if (k == "wave/fast_mode") fast_mode = b(); else if (k == "wave/cutoff_dist") cutoff_dist = fl();
        else if (k == "hash/bucket_max") max_bucket = in(); else if (k == "hash/block_max") max_block = in();
        else if (k == "gpu/wave_workgroups") wave_workgroups = in(); else if (k == "gpu/place_tries") place_tries = in();
        else if (k == "is_ext_obsv_3D") is_ext_obsv_3D = b();
    }
    gie_config to_config(int device_id = 0) const
    {
        gie_config c;
        std::memset(&c, 0, sizeof(c));
        c.voxel_width = voxel_width;
        c.local_size[0] = (int)(local_size_x / voxel_width);      /* float → int truncation, volumetric_mapper.cpp:70 */
        c.local_size[1] = (int)(local_size_y / voxel_width);
        c.local_size[2] = (int)(local_size_z / voxel_width);
        c.occupancy_threshold = occupancy_threshold;
        c.ogm_min_h = ogm_min_h; c.ogm_max_h = ogm_max_h;
        c.cutoff_grids_sq = cutoff_grids_sq();
        c.fast_mode = fast_mode; c.for_motion_planner = for_motion_planner; c.robot_r2_grids = robot_r2_grids();
        c.max_blocks = 0;            /* hash/block_max of the shipped yaml files (≈12-22 k) is far too small for big volumes */
        c.device_id = device_id;
        c.wave_workgroups = wave_workgroups; c.place_tries = place_tries;
        return c;
    }
};

/* ---------------------------------------------------------------- sensor adapters */
struct PointXYZIR { float x, y, z, intensity; uint16_t ring; };

class Vlp16Adapter {
public:
    explicit Vlp16Adapter(const gie_multiscan_param &p = { 440, 16, 10.f, (float)(2.0 * M_PI / 440), (float)-M_PI, (float)(2.0 / 180.0 * M_PI), (float)(-15.0 / 180.0 * M_PI) },
                          bool use_rs_lidar = false)
        : p_(p), rs_(use_rs_lidar), ranges_((size_t)p.scan_num * p.ring_num) {}
    /* ring binning of one cloud: ranges[ring][bin] = horizontal range, +inf where nothing fell */
    const float *convert(const PointXYZIR *pts, size_t n)
    {
        std::fill(ranges_.begin(), ranges_.end(), std::numeric_limits<float>::infinity());
        const float res = std::fabs(p_.theta_inc);
        for (size_t i = 0; i < n; i++) {
            uint16_t r = pts[i].ring;
            if (rs_ && r >= 8) r = (uint16_t)(23 - r);            /* USE_RS_LIDAR remap */
            if (r >= p_.ring_num) continue;
            const int bin = (int)((atan2f(pts[i].y, pts[i].x) + (float)M_PI) / res);
            if (bin >= 0 && bin < p_.scan_num) ranges_[(size_t)r * p_.scan_num + bin] = sqrtf(pts[i].x * pts[i].x + pts[i].y * pts[i].y);
        }
        return ranges_.data();
    }
    const gie_multiscan_param &param() const { return p_; }
private:
    gie_multiscan_param p_;
    bool rs_;
    std::vector<float> ranges_;
};

class PointCloudAdapter {
public:
    explicit PointCloudAdapter(size_t cld_sz) : cap_(cld_sz), xyz_(cld_sz * 3) {}
    /* keeps at most cld_sz points, in order */
    size_t process(const float *xyz, size_t n)
    {
        const size_t m = std::min(n, cap_);
        std::memcpy(xyz_.data(), xyz, m * 3 * sizeof(float));
        return valid_ = m;
    }
    const float *data() const { return xyz_.data(); }
    size_t valid() const { return valid_; }
private:
    size_t cap_, valid_ = 0;
    std::vector<float> xyz_;
};

/* ---------------------------------------------------------------- external obstacles */
class ExtObstacles {
public:
    void assign_premap(const std::vector<Vec3> &ll, const std::vector<Vec3> &ur) { ll_ = ll; ur_ = ur; }
    void append(const Vec3 &ll, const Vec3 &ur) { ll_.push_back(ll); ur_.push_back(ur); }
    static bool intersects(const Vec3 &a_ll, const Vec3 &a_ur, const Vec3 &b_ll, const Vec3 &b_ur)
    {
        return a_ll.x <= b_ur.x && a_ur.x >= b_ll.x && a_ll.y <= b_ur.y && a_ur.y >= b_ll.y && a_ll.z <= b_ur.z && a_ur.z >= b_ll.z;
    }
    /* box 0 (the fence) is never active; the others are active when they touch the local volume */
    void activate(const Vec3 &loc_ll, const Vec3 &loc_ur)
    {
        act_.assign(ll_.size(), 0);
        for (size_t i = 1; i < ll_.size(); i++) act_[i] = intersects(loc_ll, loc_ur, ll_[i], ur_[i]) ? 1 : 0;
    }
    int upload(gie_mapper *m) const
    {
        return gie_set_ext_boxes(m, ll_.empty() ? nullptr : &ll_[0].x, ur_.empty() ? nullptr : &ur_[0].x, act_.empty() ? nullptr : act_.data(), (int)ll_.size());
    }
    size_t size() const { return ll_.size(); }
    const Vec3 &ll(size_t i) const { return ll_[i]; }
    const Vec3 &ur(size_t i) const { return ur_[i]; }
    const std::vector<uint8_t> &active() const { return act_; }

    /* Density clustering of the external cloud (VOLMAPNODE::clustring): neighbourhood radius
     * 0.3 m; a point seeds a group with everything in its neighbourhood, and the group keeps
     * growing through members that have >= 3 neighbours (themselves included); groups of >= 4
     * points become one axis-aligned box each.  z extent is fixed to [0.2, 2.6] unless is_3d.
     * Neighbour search: uniform buckets of one radius, so a query looks at 27 buckets. */
    void cluster_cloud(const float *xyz, size_t n, bool is_3d, const std::vector<Vec3> &pre_ll, const std::vector<Vec3> &pre_ur)
    {
        assign_premap(pre_ll, pre_ur);
        if (n == 0) return;
        const float rad = 0.3f, rad2 = rad * rad;
        const size_t min_core = 3, min_group = 4;
        struct Cell { int64_t key; int idx; };
        auto cell_of = [&](const float *p, int d) { return (int64_t)std::floor(p[d] / rad); };
        auto key_of = [](int64_t cx, int64_t cy, int64_t cz) { return ((cx & 0x1fffff) << 42) | ((cy & 0x1fffff) << 21) | (cz & 0x1fffff); };
        std::vector<Cell> cells(n);
        for (size_t i = 0; i < n; i++) cells[i] = { key_of(cell_of(xyz + 3 * i, 0), cell_of(xyz + 3 * i, 1), cell_of(xyz + 3 * i, 2)), (int)i };
        std::sort(cells.begin(), cells.end(), [](const Cell &a, const Cell &b) { return a.key != b.key ? a.key < b.key : a.idx < b.idx; });
        auto around = [&](int i, std::vector<int> &out) {
            out.clear();
            const float *p = xyz + 3 * (size_t)i;
            const int64_t cx = cell_of(p, 0), cy = cell_of(p, 1), cz = cell_of(p, 2);
            for (int64_t dx = -1; dx <= 1; dx++) for (int64_t dy = -1; dy <= 1; dy++) for (int64_t dz = -1; dz <= 1; dz++) {
                const int64_t k = key_of(cx + dx, cy + dy, cz + dz);
                auto it = std::lower_bound(cells.begin(), cells.end(), k, [](const Cell &c, int64_t key) { return c.key < key; });
                for (; it != cells.end() && it->key == k; ++it) {
                    const float *q = xyz + 3 * (size_t)it->idx;
                    const float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
                    if (ex * ex + ey * ey + ez * ez <= rad2) out.push_back(it->idx);
                }
            }
        };
        enum : uint8_t { FRESH, PENDING, SETTLED };
        std::vector<uint8_t> mark(n, FRESH);
        std::vector<int> near, group;
        for (size_t s = 0; s < n; s++) {
            if (mark[s] == SETTLED) continue;
            group.assign(1, (int)s);
            mark[s] = SETTLED;
            around((int)s, near);
            for (int j : near) if (j != (int)s) { group.push_back(j); mark[j] = PENDING; }     /* seeds take their whole neighbourhood */
            for (size_t head = 1; head < group.size(); head++) {
                const int p = group[head];
                if (mark[p] == SETTLED) continue;
                around(p, near);
                if (near.size() >= min_core)
                    for (int j : near) if (mark[j] == FRESH) { group.push_back(j); mark[j] = PENDING; }
                mark[p] = SETTLED;
            }
            if (group.size() < min_group) continue;
            Vec3 lo{ xyz[3 * group[0]], xyz[3 * group[0] + 1], xyz[3 * group[0] + 2] }, hi = lo;
            for (int p : group) {
                const float *q = xyz + 3 * (size_t)p;
                lo.x = std::min(lo.x, q[0]); lo.y = std::min(lo.y, q[1]); lo.z = std::min(lo.z, q[2]);
                hi.x = std::max(hi.x, q[0]); hi.y = std::max(hi.y, q[1]); hi.z = std::max(hi.z, q[2]);
            }
            if (!is_3d) { lo.z = 0.2f; hi.z = 2.6f; }
            append(lo, hi);
        }
    }
private:
    std::vector<Vec3> ll_, ur_;
    std::vector<uint8_t> act_;
};

/* ---------------------------------------------------------------- CSV log */
class CsvLog {
public:
    explicit CsvLog(const std::string &path, const std::string &sep = ",") : f_(path), sep_(sep) {}
    CsvLog &operator<<(const char *s) { f_ << '"' << s << '"' << sep_; return *this; }
    CsvLog &operator<<(const std::string &s) { f_ << '"' << s << '"' << sep_; return *this; }
    template <class T> CsvLog &operator<<(const T &v) { f_ << v << sep_; return *this; }
    void endrow() { f_ << std::endl; }
    bool ok() const { return (bool)f_; }
private:
    std::ofstream f_;
    std::string sep_;
};

/* ---------------------------------------------------------------- accuracy check */
struct RmsResult { double rms, max_err; size_t less, more, n; };
/* EDT value of every known voxel against the true distance to the nearest OCCUPIED voxel of the
 * same local volume (what the KD-tree query of the reference returns), both in metres */
inline RmsResult ground_truth_check(const float *edt, const int8_t *type, int X, int Y, int Z, float voxel_width)
{
    std::vector<int> ox, oy, oz;
    for (int z = 0; z < Z; z++) for (int y = 0; y < Y; y++) for (int x = 0; x < X; x++)
        if (type[((size_t)z * Y + y) * X + x] == GIE_VOX_OCCUPIED) { ox.push_back(x); oy.push_back(y); oz.push_back(z); }
    RmsResult r{ 0, 0, 0, 0, 0 };
    if (ox.empty()) { r.rms = -1; return r; }
    double s2 = 0;
    for (int z = 0; z < Z; z++) for (int y = 0; y < Y; y++) for (int x = 0; x < X; x++) {
        const size_t id = ((size_t)z * Y + y) * X + x;
        if (type[id] == GIE_VOX_UNKNOWN) continue;
        long best = std::numeric_limits<long>::max();
        for (size_t i = 0; i < ox.size(); i++) {
            const long dx = x - ox[i], dy = y - oy[i], dz = z - oz[i];
            best = std::min(best, dx * dx + dy * dy + dz * dz);
        }
        const double err = std::sqrt((double)best) * voxel_width - (double)edt[id] * voxel_width;
        if (err > 0.001) r.less++; else if (err < -0.001) r.more++;
        s2 += err * err; r.max_err = std::max(r.max_err, std::fabs(err)); r.n++;
    }
    r.rms = r.n ? std::sqrt(s2 / (double)r.n) : -1;
    return r;
}

/* ---------------------------------------------------------------- CPU mirror of the global map */
/* What CPU planners and the RViz publishers read: block key → index into a growing array of
 * blocks; voxels inside a block in get_voxID_in_VB order.  update() pulls the blocks the device
 * flagged since the last call. */
class BlockMirror {
public:
    struct Key { int32_t x, y, z; bool operator==(const Key &o) const { return x == o.x && y == o.y && z == o.z; } };
    struct KeyHash { size_t operator()(const Key &k) const { return ((size_t)(uint32_t)k.x * 73856093u) ^ ((size_t)(uint32_t)k.y * 19349669u) ^ ((size_t)(uint32_t)k.z * 83492791u); } };
    static int vox_id(int gx, int gy, int gz) { return (gx & 7) * 64 + (gy & 7) * 8 + (gz & 7); }
    static Key key_of(int gx, int gy, int gz) { return { gx >> 3, gy >> 3, gz >> 3 }; }

    /* returns the number of blocks refreshed */
    int update(gie_mapper *m)
    {
        int32_t n = 0;
        if (gie_stream_changed(m, nullptr, nullptr, 0, &n) != GIE_OK) throw std::runtime_error(std::string("gie_stream_changed: ") + gie_last_error());
        if (n == 0) return 0;
        keys_.resize(3 * (size_t)n); vox_.resize((size_t)n * GIE_BLOCK_VOXELS);
        int32_t before = 0;
        if (gie_stream_changed(m, keys_.data(), vox_.data(), n, &before) != GIE_OK) throw std::runtime_error(std::string("gie_stream_changed: ") + gie_last_error());
        for (int i = 0; i < n; i++) {
            const Key k{ keys_[3 * i], keys_[3 * i + 1], keys_[3 * i + 2] };
            auto it = index.find(k);
            size_t slot;
            if (it == index.end()) { slot = block_keys.size(); index.emplace(k, slot); block_keys.push_back(k); blocks.resize((slot + 1) * GIE_BLOCK_VOXELS); }
            else slot = it->second;
            std::memcpy(&blocks[slot * GIE_BLOCK_VOXELS], &vox_[(size_t)i * GIE_BLOCK_VOXELS], GIE_BLOCK_VOXELS * sizeof(gie_voxel));
        }
        return n;
    }
    /* nullptr when the block was never streamed */
    const gie_voxel *find(int gx, int gy, int gz) const
    {
        auto it = index.find(key_of(gx, gy, gz));
        return it == index.end() ? nullptr : &blocks[it->second * GIE_BLOCK_VOXELS + vox_id(gx, gy, gz)];
    }
    std::unordered_map<Key, size_t, KeyHash> index;     /* hash_table_H_std */
    std::vector<Key> block_keys;                        /* VB_keys_H */
    std::vector<gie_voxel> blocks;                      /* VB_values_H */
private:
    std::vector<int32_t> keys_;
    std::vector<gie_voxel> vox_;
};

/* ---------------------------------------------------------------- the node's per-frame logic */
struct CostMap {                        /* msg/CostMap.msg */
    int32_t x_size = 0, y_size = 0, z_size = 0;
    float x_origin = 0, y_origin = 0, z_origin = 0, width = 0;
    uint8_t type = 1;                   /* TYPE_EDT */
    std::vector<gie_seendist> payload8;
};

struct Pose { float pos[3]; float quat_wxyz[4]; };

/* what VOLMAPNODE::visualize publishes (volumetric_mapper.h:181-357): x, y, z in metres; intensity = the type (2) in the two OGM
 * clouds (the reference's global one is PointXYZ: ignore it there), the distance in metres in the two EDT clouds */
struct DisplayClouds { std::vector<gie_cloud_point> loc_ogm, loc_edt, glb_ogm, glb_edt; };
/* global_frontier_blocks(): a block of the global map that still holds frontier — the world position of its first FNT voxel, how many
 * FNT voxels it has, the least squared distance (voxels) from its free space to an obstacle (GIE_EMPTY_VALUE: none known) */
struct FrontierBlockGoal { float pos[3]; int32_t key[3]; int32_t n_fnt, min_dist_sq; };
/* global_frontier_routes(): the same with the number of block links of the shortest route from the robot's block (include/gie.h
 * "global block routes"); -1: no route through mapped space */
struct FrontierRouteGoal : FrontierBlockGoal { int32_t steps; };

class VolumetricMapper {
public:
    explicit VolumetricMapper(const Parameters &p, int device_id = 0) : param(p), cfg_(p.to_config(device_id))
    {
        m_ = gie_create(&cfg_);
        if (!m_) throw std::runtime_error(std::string("gie_create: ") + gie_last_error());
        ext.assign_premap(p.obsbbx_ll, p.obsbbx_ur);
        streaming_ = p.cpu_mirror && (p.display_glb_edt || p.display_glb_ogm);       /* volumetric_mapper.cpp:182,196-198 */
        if (streaming_) chk(gie_stream_enable(m_, 1));
        if (p.for_motion_planner) {
            cost_map.x_size = cfg_.local_size[0]; cost_map.y_size = cfg_.local_size[1]; cost_map.z_size = cfg_.local_size[2];
            cost_map.payload8.resize((size_t)cfg_.local_size[0] * cfg_.local_size[1] * cfg_.local_size[2]);
        }
    }
    ~VolumetricMapper()
    {
#ifdef GIE_HOST_HAS_HIP
        if (explore_dev_) (void)hipFree(explore_dev_);
#endif
        if (m_) gie_destroy(m_);
    }
    VolumetricMapper(const VolumetricMapper &) = delete;
    VolumetricMapper &operator=(const VolumetricMapper &) = delete;

    enum Sensor { DEPTH, SCAN2D, MULTISCAN, POINTCLOUD };
    struct Frame {
        Sensor kind;
        const float *data; int n;       /* depth: rows*cols; scan2d: ranges; multiscan: ring-major image; pointcloud: n points xyz */
        gie_cam_param cam; gie_scan_param scan; gie_multiscan_param mscan;
    };

    /* VOLMAPNODE::publishMap (src/volumetric_mapper.cpp:138-224) without the ROS plumbing */
    void publishMap(Pose pose, const Frame &f)
    {
        using clk = std::chrono::steady_clock;
        if (param.ugv_height > 0) pose.pos[2] = param.ugv_height;
        auto t0 = clk::now();
        chk(gie_set_pose(m_, pose.pos, pose.quat_wxyz));
        for (int i = 0; i < 3; i++) robot_pos_[i] = pose.pos[i];
        switch (f.kind) {
        case DEPTH: chk(gie_ogm_depth(m_, f.data, &f.cam)); break;
        case SCAN2D: chk(gie_ogm_scan2d(m_, f.data, &f.scan)); break;
        case MULTISCAN: chk(gie_ogm_multiscan(m_, f.data, &f.mscan)); break;
        case POINTCLOUD: chk(gie_ogm_pointcloud(m_, f.data, f.n)); break;
        }
        /* update_ext_map (:498-508): boxes that touch the local volume become active */
        int32_t pvt[3];
        chk(gie_get_pivot(m_, pvt));                           /* _msg_origin = coord2pos(pivot) */
        const Vec3 ll{ (float)pvt[0] * param.voxel_width, (float)pvt[1] * param.voxel_width, (float)pvt[2] * param.voxel_width }, ur{ ll.x + param.local_size_x, ll.y + param.local_size_y, ll.z + param.local_size_z };
        ext.activate(ll, ur);
        chk(ext.upload(m_));
        chk(gie_fuse(m_));
        chk(gie_sync(m_));                                     /* GPU_DEV_SYNC, "only for profiling" (:186) */
        auto t1 = clk::now();
        chk(gie_batch_edt(m_));
        chk(gie_merge(m_));
        if (streaming_) streamed_blocks = mirror.update(m_);     /* streamPipeline is inside the reference's EDT timing too (:196-202) */
        chk(gie_sync(m_));
        auto t2 = clk::now();
        ogm_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        edt_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
        if (param.for_motion_planner) {
            gie_costmap_hdr h;
            chk(gie_read_costmap(m_, cost_map.payload8.data(), &h));
            cost_map.x_origin = h.x_origin; cost_map.y_origin = h.y_origin; cost_map.z_origin = h.z_origin;
            cost_map.width = h.width; cost_map.type = h.type;
        }
        frame++;
    }

    /* the signed distance field of the local volume (include/gie.h gie_read_sdf), voxel units, x fastest */
    void readSignedDistance(std::vector<float> &sdf)
    {
        sdf.resize((size_t)cfg_.local_size[0] * cfg_.local_size[1] * cfg_.local_size[2]);
        chk(gie_read_sdf(m_, sdf.data(), nullptr));
    }
    /* interpolated distance (m) and gradient (m/m, 3 per point) at n points xyz (m, world frame); flags as gie_query_sdf */
    void querySignedDistance(const float *xyz, int n, float *dist, float *grad, uint8_t *flags)
    {
        chk(gie_query_sdf(m_, xyz, n, dist, grad, flags));
    }

    /* the NF1 navigation function (include/gie.h gie_nf1_compute): steps to the nearest goal (metres, world frame, 3 per goal) or,
     * with GIE_NF1_FROM_FRONTIERS, frontier, through voxels with clearance_m of free space; -1 where none is reachable; x fastest.
     * Returns the number of sources. */
    int navigationFunction(const float *goals, int n, float clearance_m, int flags, std::vector<int32_t> &nf1)
    {
        gie_nf1_param p = {};
        p.clearance = clearance_m / cfg_.voxel_width;
        p.flags = flags;
        int32_t sources = 0;
        chk(gie_nf1_compute(m_, goals, n, &p, &sources));
        nf1.resize((size_t)cfg_.local_size[0] * cfg_.local_size[1] * cfg_.local_size[2]);
        chk(gie_read_nf1(m_, nf1.data()));
        return sources;
    }
    /* the descent from `start` (metres, world frame) in the last navigation function: global voxel coordinates, the start first,
     * the source last; empty when no source is reachable from it; at most max_len points */
    std::vector<std::array<int32_t, 3>> navigationPath(const float start[3], int max_len)
    {
        std::vector<int32_t> xyz((size_t)std::max(max_len, 1) * 3);
        int32_t len = 0;
        chk(gie_nf1_path(m_, start, 1, max_len, xyz.data(), &len));
        std::vector<std::array<int32_t, 3>> out((size_t)std::min(len, max_len));
        for (size_t i = 0; i < out.size(); i++) out[i] = { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] };
        return out;
    }

    /* the frontier clusters (include/gie.h gie_frontier_compute): the connected components (connectivity 6 or 26) of the FNT voxels
     * with clearance_m of free space, those of at least min_size voxels kept, at most max_clusters records in ascending label
     * order; goals (3 floats per record, metres, world frame) are the records' representative voxels, ready for
     * navigationFunction.  Returns the number of kept components (which may exceed max_clusters). */
    int frontierClusters(float clearance_m, int min_size, int connectivity, int max_clusters, std::vector<gie_frontier_cluster> &clusters,
                         std::vector<float> &goals)
    {
        gie_frontier_param p = {};
        p.clearance = clearance_m / cfg_.voxel_width;
        p.min_size = min_size; p.connectivity = connectivity; p.max_clusters = max_clusters;
        int32_t n = 0, voxels = 0;
        chk(gie_frontier_compute(m_, &p, &n, &voxels));
        const size_t cap = (size_t)std::max(max_clusters, 0);
        clusters.resize(std::max<size_t>(cap, 1)); goals.resize(3 * std::max<size_t>(cap, 1));
        chk(gie_read_frontier_clusters(m_, clusters.data(), goals.data(), &n));
        const size_t have = std::min<size_t>((size_t)n, cap);
        clusters.resize(have); goals.resize(3 * have);
        return n;
    }
    /* the label plane of the last frontierClusters: -1 not a frontier member, -2 filtered, otherwise the cluster's label; x fastest */
    void frontierLabels(std::vector<int32_t> &labels)
    {
        labels.resize((size_t)cfg_.local_size[0] * cfg_.local_size[1] * cfg_.local_size[2]);
        chk(gie_read_frontier_labels(m_, labels.data()));
    }

#ifdef GIE_HOST_HAS_HIP
    /* What a tour planner needs to order the frontier clusters (include/gie.h "cost matrix"): the path lengths, in voxel steps
     * through space with clearance_m of free room, among the robot (point 0: the position of the last publishMap) and the goals of
     * at most max_clusters (<= 63) frontier clusters of at least min_size voxels (connectivity 26).  Three device-side calls
     * chained on the mapper's stream — the clusters, their goals into one buffer behind the robot's position, the matrix of that
     * buffer — and ONE copy back; the host learns no count in between.
     *   goals  3 * (max_clusters + 1) floats, metres: the robot, then the goals in ascending label order, NaN beyond the clusters;
     *   cost   (max_clusters + 1)^2, row-major: -1 for a NaN entry, a goal the robot cannot reach, or a robot outside free space.
     * Returns the number of kept clusters (which may exceed max_clusters). */
    int exploration_costs(int max_clusters, float clearance_m, int min_size, std::vector<int32_t> &cost, std::vector<float> &goals)
    {
        if (max_clusters < 0 || max_clusters + 1 > GIE_COSTMAT_MAX_POINTS) throw std::invalid_argument("exploration_costs: 0 <= max_clusters <= 63");
        const size_t n = (size_t)max_clusters + 1, off_cost = n * 12, off_counts = off_cost + n * n * 4, bytes = off_counts + 8;
        if (bytes > explore_cap_) {
            if (explore_dev_) (void)hipFree(explore_dev_);
            explore_dev_ = nullptr; explore_cap_ = 0;
            if (hipMalloc(&explore_dev_, bytes) != hipSuccess) throw std::runtime_error("exploration_costs: device allocation failed");
            explore_cap_ = bytes;
        }
        void *stream = nullptr;
        chk(gie_get_stream(m_, &stream));
        char *d = static_cast<char *>(explore_dev_);
        explore_host_.resize(bytes);
        if (hipMemcpyAsync(d, robot_pos_, 12, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("exploration_costs: copy failed");
        gie_frontier_param fp = {};
        fp.clearance = clearance_m / cfg_.voxel_width;
        fp.min_size = min_size; fp.connectivity = 26; fp.max_clusters = max_clusters;
        chk(gie_frontier_compute_dev(m_, &fp, reinterpret_cast<int32_t *>(d + off_counts)));
        if (max_clusters > 0) chk(gie_read_frontier_clusters_dev(m_, nullptr, reinterpret_cast<float *>(d) + 3, nullptr));
        gie_nf1_param np = {};
        np.clearance = fp.clearance;
        chk(gie_costmat_compute_dev(m_, reinterpret_cast<const float *>(d), (int)n, &np, reinterpret_cast<int32_t *>(d + off_cost), nullptr));
        if (hipMemcpyAsync(explore_host_.data(), d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("exploration_costs: copy failed");
        chk(gie_sync(m_));
        goals.resize(3 * n); cost.resize(n * n);
        std::memcpy(goals.data(), explore_host_.data(), off_cost);
        std::memcpy(cost.data(), explore_host_.data() + off_cost, n * n * 4);
        int32_t counts[2];
        std::memcpy(counts, explore_host_.data() + off_counts, 8);
        return counts[0];
    }
#endif

    /* line of sight (include/gie.h gie_los_prepare): the opaque plane of the current map — OCCUPIED, UNKNOWN too with
     * GIE_LOS_UNKNOWN_OPAQUE, and everything closer than clearance_m to an obstacle; returns the number of opaque voxels.
     * lineOfSight / viewGain refer to it until the next call, whatever the map does meanwhile. */
    int losPrepare(float clearance_m, int flags)
    {
        gie_los_param p = {};
        p.clearance = clearance_m / cfg_.voxel_width;
        p.flags = flags;
        int32_t n = 0;
        chk(gie_los_prepare(m_, &p, &n));
        return n;
    }
    /* n segments a -> b (3 floats per point, metres, world frame): first opaque voxel, length, minimum clearance along each */
    void lineOfSight(const float *a_xyz, const float *b_xyz, int n, std::vector<gie_los_hit> &hits)
    {
        hits.resize((size_t)std::max(n, 0));
        chk(gie_los_segments(m_, a_xyz, b_xyz, n, hits.data()));
    }
    /* what a sensor of range [r_min_m, r_max_m] (tan2_elev < 0: no vertical band) would see from each view: the visible UNKNOWN,
     * FNT and OCCUPIED voxels and the number of candidates */
    void viewGain(const std::vector<gie_view> &views, float r_min_m, float r_max_m, float tan2_elev, std::vector<gie_view_score> &scores)
    {
        gie_view_param vp = {};
        vp.r_min = r_min_m; vp.r_max = r_max_m; vp.tan2_elev = tan2_elev;
        scores.resize(views.size());
        chk(gie_view_gain(m_, views.data(), (int)views.size(), &vp, scores.data()));
    }

    /* The 2-D CostMap a ground planner takes beside ugv_height (include/gie.h "ground costmap"): the columns of the band
     * [ground_min_height, ground_max_height] of the map as it stands and their exact distance transform, as a one-layer TYPE_EDT
     * map of X * Y elements.  Returns false, and leaves both arguments alone, while the band is not set. */
    bool ground_costmap(std::vector<gie_seendist> &payload, gie_costmap_hdr &hdr)
    {
        if (param.ground_max_height < param.ground_min_height) return false;
        const float w = cfg_.voxel_width;
        gie_ground_param p = {};
        p.z_lo = (int32_t)std::floor(param.ground_min_height / w + 0.5f);      /* gie_pos2coord, in fp32 */
        p.z_hi = (int32_t)std::floor(param.ground_max_height / w + 0.5f);
        p.min_known = param.ground_min_known;
        chk(gie_ground_compute(m_, &p, ground_counts));
        payload.resize((size_t)cfg_.local_size[0] * cfg_.local_size[1]);
        chk(gie_read_costmap_ground(m_, payload.data(), &hdr));
        return true;
    }
    int32_t ground_counts[4] = { 0, 0, 0, 0 };   /* columns of the last ground_costmap(): UNKNOWN, FREE, OCCUPIED, FNT */

    /* What an optimising planner takes from that CostMap (include/gie.h "ground signed distance"): at n points xy (metres, world
     * frame, two floats each) the bilinear signed distance (metres; negative inside an obstacle, NaN outside the field) and its
     * gradient (m/m, two per point), on the ground field ground_costmap() left.  Returns false, and leaves both arguments alone,
     * while the band is not set. */
    bool ground_distance(const float *xy, int n, std::vector<float> &dist, std::vector<float> &grad)
    {
        if (param.ground_max_height < param.ground_min_height) return false;
        dist.resize((size_t)std::max(n, 0));
        grad.resize((size_t)std::max(n, 0) * 2);
        if (n > 0) chk(gie_ground_query_sdf(m_, xy, n, dist.data(), grad.data(), nullptr));
        return true;
    }

    /* gie_ground_nf1_param.clearance_sq of ground_robot_radius: cells = ceil(radius / voxel_width), squared */
    int ground_clearance_sq() const { const int cells = (int)ceilf(param.ground_robot_radius / cfg_.voxel_width); return cells * cells; }
    /* A ground robot's plan on the map as it stands (include/gie.h "ground navigation function"): the ground field of the band as
     * ground_costmap() computes it, its NF1 from n goals (metres, world frame, two floats each) or, with from_frontiers, from the
     * field's FNT cells too, at the clearance of ground_robot_radius, and ONE descent from the robot's position of the last
     * publishMap: at most max_len points, GLOBAL cell x, y, the robot's cell first; empty when no source can be reached.
     * ground_plan_len = the descent's full length (steps + 1; it exceeds path.size() when max_len cut it), ground_plan_sources =
     * the number of sources.  Returns false, and leaves everything alone, while the band is not set. */
    bool ground_plan(const float *goal_xy, int n, bool from_frontiers, int max_len, std::vector<std::array<int32_t, 2>> &path)
    {
        if (param.ground_max_height < param.ground_min_height) return false;
        const float w = cfg_.voxel_width;
        gie_ground_param g = {};
        g.z_lo = (int32_t)std::floor(param.ground_min_height / w + 0.5f);      /* as ground_costmap() */
        g.z_hi = (int32_t)std::floor(param.ground_max_height / w + 0.5f);
        g.min_known = param.ground_min_known;
        chk(gie_ground_compute(m_, &g, ground_counts));
        gie_ground_nf1_param p = {};
        p.clearance_sq = ground_clearance_sq();
        p.flags = from_frontiers ? GIE_GROUND_NF1_FROM_FRONTIERS : 0;
        chk(gie_ground_nf1_compute(m_, goal_xy, n, &p, &ground_plan_sources));
        std::vector<int32_t> xy((size_t)std::max(max_len, 1) * 2);
        ground_plan_len = 0;
        chk(gie_ground_nf1_path(m_, robot_pos_, 1, max_len, xy.data(), &ground_plan_len));
        path.resize((size_t)std::min(ground_plan_len, max_len));
        for (size_t i = 0; i < path.size(); i++) path[i] = { xy[2 * i], xy[2 * i + 1] };
        return true;
    }
    int32_t ground_plan_len = 0, ground_plan_sources = 0;      /* of the last ground_plan() */

    /* The plan a ground robot can drive (include/gie.h "ground line of sight"): ground_plan()'s chain — the ground field, its NF1,
     * one descent of at most max_len points from the robot's position — and then the any-angle shortcut of that descent at the
     * same clearance, ground_clearance_sq(), with a look-ahead of `lookahead` path points: wp holds the waypoints, the robot's
     * cell first (every one of them: it is sized by the count), ground_waypoints_info their count, the number of forced legs (0
     * for a descent of this field) and the length in cells.  ground_plan_len and ground_plan_sources are set as by ground_plan().
     * Returns false, and leaves everything alone, while the band is not set. */
    bool ground_waypoints(const float *goal_xy, int n, bool from_frontiers, int max_len, int lookahead, std::vector<gie_ground_waypoint> &wp)
    {
        std::vector<std::array<int32_t, 2>> path;
        if (!ground_plan(goal_xy, n, from_frontiers, max_len, path)) return false;
        const int32_t len = (int32_t)path.size();
        const int cap = std::max(len, 1);
        std::vector<int32_t> xy((size_t)cap * 2, 0);
        for (size_t i = 0; i < path.size(); i++) { xy[2 * i] = path[i][0]; xy[2 * i + 1] = path[i][1]; }
        gie_ground_shortcut_param p = {};
        p.lookahead = lookahead; p.max_wp = cap; p.clearance_sq = ground_clearance_sq();
        wp.assign((size_t)cap, gie_ground_waypoint{});
        chk(gie_ground_shortcut(m_, xy.data(), &len, 1, cap, &p, wp.data(), &ground_waypoints_info));
        wp.resize((size_t)ground_waypoints_info.count);
        return true;
    }
    gie_shortcut_info ground_waypoints_info = { 0, 0, 0.f, 0 };   /* of the last ground_waypoints() */

    /* The local half of that plan (include/gie.h "ground rollouts"): n unicycle arcs of T poses from the robot's position of the
     * last publishMap at heading `yaw`, arc i driven at v[i] m/s and omega[i] rad/s in steps of dt seconds — pose 0 is the robot,
     * then x += v dt cos(theta), y += v dt sin(theta), theta += omega dt, in double, stored as float — scored by
     * gie_ground_rollouts on the ground field and NF1 that ground_plan() or ground_waypoints() left, at ground_clearance_sq(), with
     * inflate_sq = ceil(inflate_radius / voxel_width)^2 and the NF1 flag.  poses holds the n * T * 2 floats that were scored,
     * records their n records.  Returns the index of the best arc: among those with poses >= 2 and nf1_min >= 0 the least nf1_min,
     * then the least cost, then the lowest index; -1 when there is none, and -1 with everything left alone while the band is not set. */
    int ground_local_plan(float yaw, const float *v, const float *omega, int n, float dt, int T, float inflate_radius, std::vector<float> &poses,
                          std::vector<gie_ground_rollout> &records)
    {
        if (param.ground_max_height < param.ground_min_height) return -1;
        if (n < 0 || T < 1 || T > GIE_GROUND_ROLLOUT_MAX_POSES) throw std::invalid_argument("ground_local_plan: n >= 0, T in 1..4096");
        ground_arcs_(yaw, v, omega, n, dt, T, poses, nullptr);
        ground_score_arcs_(poses, n, T, inflate_radius, records);
        int best = -1;
        for (int i = 0; i < n; i++) {
            const gie_ground_rollout &r = records[(size_t)i];
            if (r.poses < 2 || r.nf1_min < 0) continue;
            if (best < 0 || r.nf1_min < records[(size_t)best].nf1_min || (r.nf1_min == records[(size_t)best].nf1_min && r.cost < records[(size_t)best].cost)) best = i;
        }
        return best;
    }

    /* The squared extents of "ground/footprint" in cells, as gie_ground_footprint_param takes them: front_sq, back_sq, side_sq, each
     * floor((metres / voxel_width)^2) in float; -1, -1, -1 while "ground/footprint" is not set (one of the three negative). */
    std::array<int32_t, 3> ground_footprint_sq() const
    {
        std::array<int32_t, 3> sq = { -1, -1, -1 };
        if (param.ground_footprint[0] < 0.f || param.ground_footprint[1] < 0.f || param.ground_footprint[2] < 0.f) return sq;
        for (int i = 0; i < 3; i++) { const float c = param.ground_footprint[i] / cfg_.voxel_width; sq[(size_t)i] = (int32_t)floorf(c * c); }
        return sq;
    }

    /* ground_local_plan() for a robot that is a rectangle (include/gie.h "ground footprints"): the same n arcs, and beside every pose
     * its heading (lround(32767 cos theta), lround(32767 sin theta)) in `headings` (n * T * 2 int32).  The arcs are scored by
     * gie_ground_rollouts exactly as ground_local_plan() scores them (records), then by gie_ground_footprints with
     * ground_footprint_sq(), the margin flag and clearance_sq = 0 (footprints: the rectangle itself, no disc around it).  Returns
     * the best arc by ground_local_plan()'s order among those it admits whose footprint record has poses >= 2 as well: as there, an
     * arc that is blocked further on is still a motion to command now, the next call looks again; -1 when there is none, and -1 with
     * everything left alone while the band or "ground/footprint" is not set. */
    int ground_local_plan_footprint(float yaw, const float *v, const float *omega, int n, float dt, int T, float inflate_radius, std::vector<float> &poses,
                                    std::vector<int32_t> &headings, std::vector<gie_ground_rollout> &records, std::vector<gie_ground_footprint> &footprints)
    {
        if (param.ground_max_height < param.ground_min_height) return -1;
        if (param.ground_footprint[0] < 0.f || param.ground_footprint[1] < 0.f || param.ground_footprint[2] < 0.f) return -1;
        if (n < 0 || T < 1 || T > GIE_GROUND_ROLLOUT_MAX_POSES) throw std::invalid_argument("ground_local_plan_footprint: n >= 0, T in 1..4096");
        ground_arcs_(yaw, v, omega, n, dt, T, poses, &headings);
        ground_score_arcs_(poses, n, T, inflate_radius, records);
        const std::array<int32_t, 3> sq = ground_footprint_sq();
        gie_ground_footprint_param p = {};
        p.front_sq = sq[0]; p.back_sq = sq[1]; p.side_sq = sq[2];
        p.clearance_sq = 0;
        p.flags = GIE_GROUND_FOOTPRINT_MARGIN;
        footprints.assign((size_t)n, gie_ground_footprint{});
        chk(gie_ground_footprints(m_, poses.data(), headings.data(), n, T, &p, footprints.data()));
        int best = -1;
        for (int i = 0; i < n; i++) {
            const gie_ground_rollout &r = records[(size_t)i];
            if (r.poses < 2 || r.nf1_min < 0 || footprints[(size_t)i].poses < 2) continue;
            if (best < 0 || r.nf1_min < records[(size_t)best].nf1_min || (r.nf1_min == records[(size_t)best].nf1_min && r.cost < records[(size_t)best].cost)) best = i;
        }
        return best;
    }

    /* The heading index of "ground pose navigation function" nearest to yaw (radians): lround(yaw / (pi / 4)) taken mod 8 into 0..7;
     * index k looks along d_k, counter-clockwise from +x. */
    static int ground_heading_index(double yaw)
    {
        const long r = std::lround(yaw / 0.78539816339744830962);
        return (int)(((r % 8) + 8) % 8);
    }

    /* ground_plan() for a robot that is a rectangle (include/gie.h "ground pose navigation function"): the ground field of the band
     * exactly as ground_plan() computes it, then the pose navigation function with ground_footprint_sq() and clearance_sq = 0 (the
     * rectangle itself, no disc around it; an extent beyond GIE_GROUND_POSE_MAX_SQ is refused by the library: the call throws) from
     * n goals — goal_yaw may be NULL, and a NaN entry means any heading; otherwise goal i counts at ground_heading_index(goal_yaw[i])
     * — or, with from_frontiers, from the FNT cells too; with `reverse` the robot may back up.  ONE descent from the robot's position
     * of the last publishMap at ground_heading_index(yaw): at most max_len triples GLOBAL cell x, y and heading index, the robot's
     * state first; empty when no source can be reached.  ground_pose_plan_len = the descent's full length (moves + 1),
     * ground_pose_plan_sources = the number of source states.  ground_plan()'s own field and results are not touched.  Returns false,
     * and leaves everything alone, while the band or "ground/footprint" is not set. */
    bool ground_plan_footprint(float yaw, const float *goal_xy, const float *goal_yaw, int n, bool from_frontiers, bool reverse, int max_len,
                               std::vector<std::array<int32_t, 3>> &path)
    {
        if (param.ground_max_height < param.ground_min_height) return false;
        if (param.ground_footprint[0] < 0.f || param.ground_footprint[1] < 0.f || param.ground_footprint[2] < 0.f) return false;
        const float w = cfg_.voxel_width;
        gie_ground_param g = {};
        g.z_lo = (int32_t)std::floor(param.ground_min_height / w + 0.5f);      /* as ground_plan() */
        g.z_hi = (int32_t)std::floor(param.ground_max_height / w + 0.5f);
        g.min_known = param.ground_min_known;
        chk(gie_ground_compute(m_, &g, ground_counts));
        const std::array<int32_t, 3> sq = ground_footprint_sq();
        gie_ground_pose_nf1_param p = {};
        p.front_sq = sq[0]; p.back_sq = sq[1]; p.side_sq = sq[2];
        p.clearance_sq = 0;
        p.flags = (from_frontiers ? GIE_GROUND_POSE_NF1_FROM_FRONTIERS : 0) | (reverse ? GIE_GROUND_POSE_NF1_REVERSE : 0);
        std::vector<int32_t> gk;
        if (goal_yaw) {
            gk.resize((size_t)std::max(n, 0));
            for (size_t i = 0; i < gk.size(); i++) gk[i] = std::isnan(goal_yaw[i]) ? -1 : ground_heading_index((double)goal_yaw[i]);
        }
        int32_t counts[2] = { 0, 0 };
        chk(gie_ground_pose_nf1_compute(m_, goal_xy, goal_yaw ? gk.data() : nullptr, n, &p, counts));
        ground_pose_plan_sources = counts[0];
        std::vector<int32_t> xyk((size_t)std::max(max_len, 1) * 3);
        const int32_t k0 = ground_heading_index((double)yaw);
        ground_pose_plan_len = 0;
        chk(gie_ground_pose_nf1_path(m_, robot_pos_, &k0, 1, max_len, xyk.data(), &ground_pose_plan_len));
        path.resize((size_t)std::min(ground_pose_plan_len, max_len));
        for (size_t i = 0; i < path.size(); i++) path[i] = { xyk[3 * i], xyk[3 * i + 1], xyk[3 * i + 2] };
        return true;
    }
    int32_t ground_pose_plan_len = 0, ground_pose_plan_sources = 0;      /* of the last ground_plan_footprint() */

#ifdef GIE_HOST_HAS_HIP
    /* A ground robot's goal selection on the map as it stands (include/gie.h "ground frontier clusters"): which frontiers exist, how
     * large they are, where to drive for each and how far that is.  Four steps chained through the _dev forms on the mapper's
     * stream, with one device buffer and ONE sync (exploration_costs' pattern; the host learns no count in between):
     *   the ground field of the band, exactly as ground_costmap() and ground_plan() set it up;
     *   its frontier clusters at ground_clearance_sq(), connectivity 8, of at least min_size cells;
     *   the ground navigation function whose one goal is the robot's position of the last publishMap (NF1 is symmetric);
     *   that field gathered at the clusters' goals.
     * clusters: the records in ascending label order, min(kept, max_clusters) of them; steps[i] = the 4-connected route length in
     * cells from the robot to clusters[i].rep, -1 for a cluster the robot cannot reach — and for ALL clusters when the robot's own
     * cell is not traversable (outside the field, not FREE or FNT, or closer than the clearance to an obstacle column): the field
     * then has no source.  ground_goals_kept = the number of kept components (which may exceed max_clusters), ground_goals_cells =
     * their members; ground_counts as by ground_costmap().  Returns false, and leaves everything alone, while the band is not set. */
    bool ground_exploration_goals(int max_clusters, int min_size, std::vector<gie_ground_frontier_cluster> &clusters, std::vector<int32_t> &steps)
    {
        if (param.ground_max_height < param.ground_min_height) return false;
        if (max_clusters < 0) throw std::invalid_argument("ground_exploration_goals: max_clusters >= 0");
        const size_t cap = (size_t)max_clusters, off_goal = cap * sizeof(gie_ground_frontier_cluster), off_robot = off_goal + cap * 8, off_steps = off_robot + 8,
                     off_counts = off_steps + cap * 4, off_ground = off_counts + 8, bytes = off_ground + 16;
        if (bytes > explore_cap_) {
            if (explore_dev_) (void)hipFree(explore_dev_);
            explore_dev_ = nullptr; explore_cap_ = 0;
            if (hipMalloc(&explore_dev_, bytes) != hipSuccess) throw std::runtime_error("ground_exploration_goals: device allocation failed");
            explore_cap_ = bytes;
        }
        void *stream = nullptr;
        chk(gie_get_stream(m_, &stream));
        char *d = static_cast<char *>(explore_dev_);
        explore_host_.resize(bytes);
        if (hipMemcpyAsync(d + off_robot, robot_pos_, 8, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("ground_exploration_goals: copy failed");
        const float w = cfg_.voxel_width;
        gie_ground_param g = {};
        g.z_lo = (int32_t)std::floor(param.ground_min_height / w + 0.5f);      /* as ground_costmap() */
        g.z_hi = (int32_t)std::floor(param.ground_max_height / w + 0.5f);
        g.min_known = param.ground_min_known;
        chk(gie_ground_compute_dev(m_, &g, reinterpret_cast<int32_t *>(d + off_ground)));
        gie_ground_frontier_param fp = {};
        fp.clearance_sq = ground_clearance_sq(); fp.min_size = min_size; fp.connectivity = 8; fp.max_clusters = max_clusters;
        chk(gie_ground_frontier_compute_dev(m_, &fp, reinterpret_cast<int32_t *>(d + off_counts)));
        float *d_goal = reinterpret_cast<float *>(d + off_goal);
        if (max_clusters > 0) chk(gie_read_ground_frontier_clusters_dev(m_, reinterpret_cast<gie_ground_frontier_cluster *>(d), d_goal, nullptr));
        gie_ground_nf1_param np = {};
        np.clearance_sq = fp.clearance_sq;
        chk(gie_ground_nf1_compute_dev(m_, reinterpret_cast<const float *>(d + off_robot), 1, &np, nullptr));
        chk(gie_ground_nf1_query_dev(m_, d_goal, max_clusters, reinterpret_cast<int32_t *>(d + off_steps)));
        if (hipMemcpyAsync(explore_host_.data(), d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("ground_exploration_goals: copy failed");
        chk(gie_sync(m_));
        int32_t counts[2];
        std::memcpy(counts, explore_host_.data() + off_counts, 8);
        std::memcpy(ground_counts, explore_host_.data() + off_ground, 16);
        ground_goals_kept = counts[0]; ground_goals_cells = counts[1];
        const size_t have = std::min<size_t>((size_t)counts[0], cap);
        clusters.resize(have); steps.resize(have);
        if (have) {
            std::memcpy(clusters.data(), explore_host_.data(), have * sizeof(gie_ground_frontier_cluster));
            std::memcpy(steps.data(), explore_host_.data() + off_steps, have * 4);
        }
        return true;
    }
    int32_t ground_goals_kept = 0, ground_goals_cells = 0;     /* of the last ground_exploration_goals() */

    /* Both halves of a ground explorer's utility in one chain (include/gie.h "ground view gain"): ground_exploration_goals()' four
     * steps with gie_ground_view_gain_dev at the clusters' goal array appended on the stream — every cell within r_min .. r_max
     * metres of a goal, in all directions (no half planes, UNKNOWN columns transparent).  Still one device buffer and ONE sync; the
     * host learns no count in between (the NaN tail of the goal array scores -1 on the device and is cut off here).
     * clusters and steps as by ground_exploration_goals(); scores[i] belongs to clusters[i]: the visible UNKNOWN / FNT / OCCUPIED
     * columns around clusters[i].rep and the number of candidates.  ground_goals_kept, ground_goals_cells and ground_counts are set
     * as there.  Returns false, and leaves everything alone, while the band is not set. */
    bool ground_exploration_gains(int max_clusters, int min_size, float r_min, float r_max, std::vector<gie_ground_frontier_cluster> &clusters,
                                  std::vector<int32_t> &steps, std::vector<gie_view_score> &scores)
    {
        if (param.ground_max_height < param.ground_min_height) return false;
        if (max_clusters < 0) throw std::invalid_argument("ground_exploration_gains: max_clusters >= 0");
        const size_t cap = (size_t)max_clusters, off_goal = cap * sizeof(gie_ground_frontier_cluster), off_robot = off_goal + cap * 8, off_steps = off_robot + 8,
                     off_counts = off_steps + cap * 4, off_ground = off_counts + 8, off_scores = off_ground + 16, bytes = off_scores + cap * sizeof(gie_view_score);
        if (bytes > explore_cap_) {
            if (explore_dev_) (void)hipFree(explore_dev_);
            explore_dev_ = nullptr; explore_cap_ = 0;
            if (hipMalloc(&explore_dev_, bytes) != hipSuccess) throw std::runtime_error("ground_exploration_gains: device allocation failed");
            explore_cap_ = bytes;
        }
        void *stream = nullptr;
        chk(gie_get_stream(m_, &stream));
        char *d = static_cast<char *>(explore_dev_);
        explore_host_.resize(bytes);
        if (hipMemcpyAsync(d + off_robot, robot_pos_, 8, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("ground_exploration_gains: copy failed");
        const float w = cfg_.voxel_width;
        gie_ground_param g = {};
        g.z_lo = (int32_t)std::floor(param.ground_min_height / w + 0.5f);      /* as ground_costmap() */
        g.z_hi = (int32_t)std::floor(param.ground_max_height / w + 0.5f);
        g.min_known = param.ground_min_known;
        chk(gie_ground_compute_dev(m_, &g, reinterpret_cast<int32_t *>(d + off_ground)));
        gie_ground_frontier_param fp = {};
        fp.clearance_sq = ground_clearance_sq(); fp.min_size = min_size; fp.connectivity = 8; fp.max_clusters = max_clusters;
        chk(gie_ground_frontier_compute_dev(m_, &fp, reinterpret_cast<int32_t *>(d + off_counts)));
        float *d_goal = reinterpret_cast<float *>(d + off_goal);
        if (max_clusters > 0) chk(gie_read_ground_frontier_clusters_dev(m_, reinterpret_cast<gie_ground_frontier_cluster *>(d), d_goal, nullptr));
        gie_ground_nf1_param np = {};
        np.clearance_sq = fp.clearance_sq;
        chk(gie_ground_nf1_compute_dev(m_, reinterpret_cast<const float *>(d + off_robot), 1, &np, nullptr));
        chk(gie_ground_nf1_query_dev(m_, d_goal, max_clusters, reinterpret_cast<int32_t *>(d + off_steps)));
        gie_ground_view_param vp = {};
        vp.r_min = r_min; vp.r_max = r_max;
        chk(gie_ground_view_gain_dev(m_, d_goal, nullptr, max_clusters, &vp, reinterpret_cast<gie_view_score *>(d + off_scores)));
        if (hipMemcpyAsync(explore_host_.data(), d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("ground_exploration_gains: copy failed");
        chk(gie_sync(m_));
        int32_t counts[2];
        std::memcpy(counts, explore_host_.data() + off_counts, 8);
        std::memcpy(ground_counts, explore_host_.data() + off_ground, 16);
        ground_goals_kept = counts[0]; ground_goals_cells = counts[1];
        const size_t have = std::min<size_t>((size_t)counts[0], cap);
        clusters.resize(have); steps.resize(have); scores.resize(have);
        if (have) {
            std::memcpy(clusters.data(), explore_host_.data(), have * sizeof(gie_ground_frontier_cluster));
            std::memcpy(steps.data(), explore_host_.data() + off_steps, have * 4);
            std::memcpy(scores.data(), explore_host_.data() + off_scores, have * sizeof(gie_view_score));
        }
        return true;
    }

    /* What a ground robot's tour planner needs to order the frontier clusters (include/gie.h "ground cost matrix"): the 4-connected
     * route lengths in cells, at ground_clearance_sq(), among the robot (point 0: the position of the last publishMap) and the goals
     * of at most max_clusters (<= 255) ground frontier clusters of at least min_size cells (connectivity 8).  ground_exploration_goals'
     * chain with exploration_costs' pattern: the ground field of the band, its frontier clusters, their goals into one device buffer
     * directly behind the robot's position, the matrix of that buffer — ONE copy back and ONE sync; the host learns no count in
     * between.
     *   goals  2 * (max_clusters + 1) floats, metres: the robot, then the goals in ascending label order, NaN beyond the clusters;
     *   cost   (max_clusters + 1)^2, row-major: -1 for a NaN entry, a goal the robot cannot reach, or a robot whose own cell is not
     *          traversable (row and column 0 are then all -1).
     * ground_goals_kept, ground_goals_cells and ground_counts are set as by ground_exploration_goals().  Returns false, and leaves
     * everything alone, while the band is not set. */
    bool ground_exploration_costs(int max_clusters, int min_size, std::vector<int32_t> &cost, std::vector<float> &goals)
    {
        if (param.ground_max_height < param.ground_min_height) return false;
        if (max_clusters < 0 || max_clusters + 1 > GIE_GROUND_COSTMAT_MAX_POINTS) throw std::invalid_argument("ground_exploration_costs: 0 <= max_clusters <= 255");
        const size_t n = (size_t)max_clusters + 1, off_cost = n * 8, off_counts = off_cost + n * n * 4, off_ground = off_counts + 8, bytes = off_ground + 16;
        if (bytes > explore_cap_) {
            if (explore_dev_) (void)hipFree(explore_dev_);
            explore_dev_ = nullptr; explore_cap_ = 0;
            if (hipMalloc(&explore_dev_, bytes) != hipSuccess) throw std::runtime_error("ground_exploration_costs: device allocation failed");
            explore_cap_ = bytes;
        }
        void *stream = nullptr;
        chk(gie_get_stream(m_, &stream));
        char *d = static_cast<char *>(explore_dev_);
        explore_host_.resize(bytes);
        if (hipMemcpyAsync(d, robot_pos_, 8, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("ground_exploration_costs: copy failed");
        const float w = cfg_.voxel_width;
        gie_ground_param g = {};
        g.z_lo = (int32_t)std::floor(param.ground_min_height / w + 0.5f);      /* as ground_costmap() */
        g.z_hi = (int32_t)std::floor(param.ground_max_height / w + 0.5f);
        g.min_known = param.ground_min_known;
        chk(gie_ground_compute_dev(m_, &g, reinterpret_cast<int32_t *>(d + off_ground)));
        gie_ground_frontier_param fp = {};
        fp.clearance_sq = ground_clearance_sq(); fp.min_size = min_size; fp.connectivity = 8; fp.max_clusters = max_clusters;
        chk(gie_ground_frontier_compute_dev(m_, &fp, reinterpret_cast<int32_t *>(d + off_counts)));
        if (max_clusters > 0) chk(gie_read_ground_frontier_clusters_dev(m_, nullptr, reinterpret_cast<float *>(d) + 2, nullptr));
        gie_ground_nf1_param np = {};
        np.clearance_sq = fp.clearance_sq;
        chk(gie_ground_costmat_compute_dev(m_, reinterpret_cast<const float *>(d), (int)n, &np, reinterpret_cast<int32_t *>(d + off_cost), nullptr));
        if (hipMemcpyAsync(explore_host_.data(), d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) throw std::runtime_error("ground_exploration_costs: copy failed");
        chk(gie_sync(m_));
        goals.resize(2 * n); cost.resize(n * n);
        std::memcpy(goals.data(), explore_host_.data(), off_cost);
        std::memcpy(cost.data(), explore_host_.data() + off_cost, n * n * 4);
        int32_t counts[2];
        std::memcpy(counts, explore_host_.data() + off_counts, 8);
        std::memcpy(ground_counts, explore_host_.data() + off_ground, 16);
        ground_goals_kept = counts[0]; ground_goals_cells = counts[1];
        return true;
    }
#endif

    /* Far exploration goals (include/gie.h "global block summaries"): the blocks of everything mapped so far — not of the local
     * volume only — that hold at least min_fnt FNT voxels (below 1: explore/min_fnt), from ONE gie_blocks_summary call with
     * GIE_BLOCKS_DIST (and one that counts).  Sorted by the squared block distance from the robot's block (its position of the last
     * publishMap), ties by key (z, y, x); at most max_goals of them.  A goal's position is coord2pos of the block's fnt_voxel, the
     * convention of the frontier clusters' goals.  Returns the number of such blocks (which may exceed max_goals). */
    int global_frontier_blocks(int min_fnt, int max_goals, std::vector<FrontierBlockGoal> &goals)
    {
        gie_blocks_param p = {};
        for (int i = 0; i < 3; i++) { p.lo[i] = std::numeric_limits<int32_t>::min(); p.hi[i] = std::numeric_limits<int32_t>::max(); }
        p.flags = GIE_BLOCKS_DIST;
        p.min_fnt = std::max(min_fnt < 1 ? param.explore_min_fnt : min_fnt, 1);
        int32_t n = 0;
        chk(gie_blocks_summary(m_, &p, nullptr, &n, nullptr));
        std::vector<gie_block_summary> rec((size_t)n);
        p.max_records = n;
        if (n > 0) chk(gie_blocks_summary(m_, &p, rec.data(), &n, nullptr));
        rec.resize((size_t)std::min<int32_t>(n, p.max_records));
        const float w = cfg_.voxel_width;
        int64_t rb[3];
        for (int i = 0; i < 3; i++) rb[i] = (int64_t)((int32_t)std::floor(robot_pos_[i] / w + 0.5f) >> 3);      /* gie_pos2coord, in fp32; its block */
        auto d2 = [&](const gie_block_summary &r) { int64_t s = 0; for (int i = 0; i < 3; i++) { const int64_t d = (int64_t)r.key[i] - rb[i]; s += d * d; } return s; };
        std::sort(rec.begin(), rec.end(), [&](const gie_block_summary &a, const gie_block_summary &b) {
            const int64_t da = d2(a), db = d2(b);
            if (da != db) return da < db;
            if (a.key[2] != b.key[2]) return a.key[2] < b.key[2];
            if (a.key[1] != b.key[1]) return a.key[1] < b.key[1];
            return a.key[0] < b.key[0];
        });
        goals.clear();
        for (size_t i = 0; i < rec.size() && (int)i < max_goals; i++) {
            const gie_block_summary &r = rec[i];
            const int v[3] = { r.fnt_voxel >> 6, (r.fnt_voxel >> 3) & 7, r.fnt_voxel & 7 };
            FrontierBlockGoal g;
            for (int k = 0; k < 3; k++) { g.key[k] = r.key[k]; g.pos[k] = (float)(r.key[k] * 8 + v[k]) * w; }
            g.n_fnt = r.n_fnt; g.min_dist_sq = r.min_dist_sq;
            goals.push_back(g);
        }
        return n;
    }

    /* The far exploration goals by ROUTE (include/gie.h "global block routes"): the goals of global_frontier_blocks(0, max_goals)
     * (explore/min_fnt), then ONE gie_routes_compute with the robot's position as the only goal and ONE gie_routes_query at the goals'
     * positions.  Nodes and links by explore/route_min_free and explore/route_min_open.  The box is the bounding box of the goals' keys
     * and the robot's block, widened by one block; if that exceeds the stage's size limit (16384 words of 64 cells a plane) it is cut
     * to the robot's block +- h on every axis, h halving from the longest reach of the box until it fits — goals beyond it are then
     * unreachable by definition.  The goals come ordered by steps, ascending; the unreachable ones (steps -1) last; ties, and the
     * unreachable among themselves, stay in global_frontier_blocks' straight-line order.  Returns its count of frontier blocks. */
    int global_frontier_routes(int max_goals, std::vector<FrontierRouteGoal> &goals)
    {
        std::vector<FrontierBlockGoal> far;
        const int n = global_frontier_blocks(0, max_goals, far);
        const float w = cfg_.voxel_width;
        gie_routes_param p = {};
        int64_t rb[3], lo[3], hi[3];
        for (int i = 0; i < 3; i++) {
            rb[i] = (int64_t)((int32_t)std::floor(robot_pos_[i] / w + 0.5f) >> 3);      /* gie_pos2coord, in fp32; its block */
            lo[i] = hi[i] = rb[i];
            for (const FrontierBlockGoal &g : far) { lo[i] = std::min<int64_t>(lo[i], g.key[i]); hi[i] = std::max<int64_t>(hi[i], g.key[i]); }
            lo[i] -= 1; hi[i] += 1;
        }
        auto words = [&]() { return ((hi[0] - lo[0] + 1 + 63) / 64) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1); };
        int64_t h = 0;
        for (int i = 0; i < 3; i++) h = std::max(h, std::max(rb[i] - lo[i], hi[i] - rb[i]));
        while (words() > 16384) {
            h /= 2;
            for (int i = 0; i < 3; i++) { lo[i] = std::max(lo[i], rb[i] - h); hi[i] = std::min(hi[i], rb[i] + h); }
        }
        for (int i = 0; i < 3; i++) { p.lo[i] = (int32_t)lo[i]; p.hi[i] = (int32_t)hi[i]; }
        p.min_free = param.explore_route_min_free; p.min_open = param.explore_route_min_open; p.min_fnt = std::max(param.explore_min_fnt, 1);
        chk(gie_routes_compute(m_, robot_pos_, 1, &p, nullptr));
        std::vector<float> xyz(3 * far.size());
        std::vector<int32_t> steps(far.size(), -1);
        for (size_t i = 0; i < far.size(); i++) for (int k = 0; k < 3; k++) xyz[3 * i + k] = far[i].pos[k];
        if (!far.empty()) chk(gie_routes_query(m_, xyz.data(), (int)far.size(), steps.data()));
        std::vector<size_t> order(far.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            const int64_t sa = steps[a] < 0 ? std::numeric_limits<int64_t>::max() : steps[a], sb = steps[b] < 0 ? std::numeric_limits<int64_t>::max() : steps[b];
            return sa < sb;
        });
        goals.clear();
        for (size_t i : order) {
            FrontierRouteGoal g;
            static_cast<FrontierBlockGoal &>(g) = far[i];
            g.steps = steps[i];
            goals.push_back(g);
        }
        return n;
    }

    /* VOLMAPNODE::visualize without the publishers: the clouds the display flags ask for (the others come back empty), of the map as
     * it stands.  sensor_pos is the reference's argument: its z is replaced by vis_height before the slice's z is taken
     * (volumetric_mapper.h:339-341), so only vis_height decides.  The local clouds always come from the device (gie_cloud_local);
     * the global ones from the mirror (cpu_mirror, the reference's loop over its blocks) or from the device (gie_cloud_global). */
    const DisplayClouds &visualize(const float sensor_pos[3])
    {
        (void)sensor_pos;
        const float w = cfg_.voxel_width;
        const uint32_t occ = 1u << GIE_VOX_OCCUPIED, known = (1u << GIE_VOX_FREE) | (1u << GIE_VOX_OCCUPIED) | (1u << GIE_VOX_FNT);
        const int32_t none_lo = std::numeric_limits<int32_t>::min(), none_hi = std::numeric_limits<int32_t>::max();
        const int32_t slice = (int32_t)std::floor(param.vis_height / w + 0.5f);      /* gie_pos2coord(vis_height, w), in fp32 */
        clouds.loc_ogm.clear(); clouds.loc_edt.clear(); clouds.glb_ogm.clear(); clouds.glb_edt.clear();
        if (param.display_loc_ogm) cloud(gie_cloud_local, occ, GIE_CLOUD_TYPE, none_lo, none_hi, clouds.loc_ogm);
        if (param.display_loc_edt) cloud(gie_cloud_local, known, GIE_CLOUD_DIST, none_lo, none_hi, clouds.loc_edt);
        if (!param.cpu_mirror) {
            if (param.display_glb_ogm) cloud(gie_cloud_global, occ, GIE_CLOUD_TYPE, none_lo, none_hi, clouds.glb_ogm);
            if (param.display_glb_edt) cloud(gie_cloud_global, known, GIE_CLOUD_DIST, slice, slice, clouds.glb_edt);
        } else if (param.display_glb_ogm || param.display_glb_edt) {      /* publish_glb_2_rviz */
            for (size_t b = 0; b < mirror.block_keys.size(); b++) {
                const BlockMirror::Key k = mirror.block_keys[b];
                for (int i = 0; i < GIE_BLOCK_VOXELS; i++) {
                    const gie_voxel &v = mirror.blocks[b * GIE_BLOCK_VOXELS + i];
                    if (v.vox_type == GIE_VOX_UNKNOWN) continue;
                    const int g[3] = { k.x * 8 + (i >> 6), k.y * 8 + ((i >> 3) & 7), k.z * 8 + (i & 7) };
                    const gie_cloud_point pt = { (float)g[0] * w, (float)g[1] * w, (float)g[2] * w, (float)v.vox_type };
                    if (param.display_glb_ogm && v.vox_type == GIE_VOX_OCCUPIED) clouds.glb_ogm.push_back(pt);
                    if (!param.display_glb_edt || g[2] != slice || v.dist_sq < 0 || v.dist_sq >= 900000) continue;     /* invalid_dist_glb */
                    clouds.glb_edt.push_back({ pt.x, pt.y, pt.z, sqrtf((float)v.dist_sq) * w });
                }
            }
        }
        return clouds;
    }
    DisplayClouds clouds;

    gie_mapper *handle() { return m_; }
    const gie_config &config() const { return cfg_; }

    Parameters param;
    ExtObstacles ext;
    BlockMirror mirror;
    int streamed_blocks = 0;
    CostMap cost_map;
    double ogm_ms = 0, edt_ms = 0;
    int frame = 0;
private:
    static void chk(int rc) { if (rc != GIE_OK) throw std::runtime_error(std::string("gie: ") + gie_last_error()); }
    /* one display cloud: count, then fetch */
    template <class F> void cloud(F fn, uint32_t mask, int intensity, int32_t z_lo, int32_t z_hi, std::vector<gie_cloud_point> &out)
    {
        gie_cloud_param p = {};
        p.type_mask = mask; p.intensity = intensity; p.z_lo = z_lo; p.z_hi = z_hi;
        int32_t n = 0;
        chk(fn(m_, &p, nullptr, &n));
        out.resize((size_t)n);
        if (n == 0) return;
        p.max_points = n;
        chk(fn(m_, &p, out.data(), &n));
    }
    gie_config cfg_;
    gie_mapper *m_ = nullptr;
    float robot_pos_[3] = { 0.f, 0.f, 0.f };      /* of the last publishMap (after ugv_height) */

    /* the arcs of ground_local_plan(): pose 0 is the robot, then x += v dt cos(theta), y += v dt sin(theta), theta += omega dt, in
     * double, stored as float; with `headings` the heading of every pose too */
    void ground_arcs_(float yaw, const float *v, const float *omega, int n, float dt, int T, std::vector<float> &poses, std::vector<int32_t> *headings) const
    {
        poses.resize((size_t)n * T * 2);
        if (headings) headings->resize((size_t)n * T * 2);
        for (int i = 0; i < n; i++) {
            double x = robot_pos_[0], y = robot_pos_[1], th = yaw;
            for (int k = 0; k < T; k++) {
                float *q = poses.data() + 2 * ((size_t)i * T + k);
                q[0] = (float)x; q[1] = (float)y;
                if (headings) {
                    int32_t *h = headings->data() + 2 * ((size_t)i * T + k);
                    h[0] = (int32_t)std::lround(32767.0 * std::cos(th)); h[1] = (int32_t)std::lround(32767.0 * std::sin(th));
                }
                x += (double)v[i] * dt * std::cos(th); y += (double)v[i] * dt * std::sin(th);
                th += (double)omega[i] * dt;
            }
        }
    }
    /* ground_local_plan()'s scoring: gie_ground_rollouts at ground_clearance_sq() with the NF1 flag */
    void ground_score_arcs_(const std::vector<float> &poses, int n, int T, float inflate_radius, std::vector<gie_ground_rollout> &records)
    {
        gie_ground_rollout_param p = {};
        p.clearance_sq = ground_clearance_sq();
        const int cells = (int)ceilf(inflate_radius / cfg_.voxel_width);
        p.inflate_sq = cells * cells;
        p.flags = GIE_GROUND_ROLLOUT_NF1;
        records.assign((size_t)n, gie_ground_rollout{});
        chk(gie_ground_rollouts(m_, poses.data(), n, T, &p, records.data()));
    }
    void *explore_dev_ = nullptr; size_t explore_cap_ = 0;     /* exploration_costs' device buffer and its host copy */
    std::vector<char> explore_host_;
    bool streaming_ = false;
};

} /* namespace gie_host */
#endif /* GIE_HOST_HPP */
