/* Test helper (tests/test_ground_los_gpu.py): VolumetricMapper::ground_waypoints over a few point-cloud frames, the last result as raw files.
 *   ground_waypoints_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 *                          <robot_radius> <from_frontiers 0|1> <max_len> <lookahead> [goal_x goal_y]...
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.wp (gie_ground_waypoint records) and <prefix>.info (int32: count, forced, the bits of length, len, sources,
 * clearance_sq) after the last frame; ground_waypoints() is also called after every earlier frame.  With max < min it must return
 * false and write nothing into `wp`. */
#include <cstring>

#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc < 15 || (argc - 15) % 2) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known radius frontiers max_len lookahead [gx gy]...\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("ground/robot_radius", argv[11]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const bool frontiers = std::stoi(argv[12]) != 0;
        const int max_len = std::stoi(argv[13]), lookahead = std::stoi(argv[14]);
        std::vector<float> goals;
        for (int i = 15; i < argc; i++) goals.push_back(std::stof(argv[i]));
        gie_host::VolumetricMapper vm(p);
        gie_ground_waypoint poison;
        memset(&poison, 0x5a, sizeof(poison));
        std::vector<gie_ground_waypoint> wp(2, poison);
        int made = 0;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_waypoints(goals.data(), (int)goals.size() / 2, frontiers, max_len, lookahead, wp) ? 1 : 0;
        }
        const std::string out = argv[2];
        int32_t length_bits;
        memcpy(&length_bits, &vm.ground_waypoints_info.length, 4);
        const int32_t info[6] = { vm.ground_waypoints_info.count, vm.ground_waypoints_info.forced, length_bits, vm.ground_plan_len, vm.ground_plan_sources,
                                  vm.ground_clearance_sq() };
        dump(out + ".wp", wp.data(), wp.size() * sizeof(wp[0]));
        dump(out + ".info", info, sizeof(info));
        printf("frames %d made %d waypoints %zu\n", in.frames, made, wp.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_waypoints_probe: %s\n", e.what()); return 1; }
    return 0;
}
