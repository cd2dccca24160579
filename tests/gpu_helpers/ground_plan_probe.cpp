/* Test helper (tests/test_ground_nf1_gpu.py): VolumetricMapper::ground_plan over a few point-cloud frames, the last plan as raw files.
 *   ground_plan_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 *                     <robot_radius> <from_frontiers 0|1> <max_len> [goal_x goal_y]...
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.path (int32 x, y per point) and <prefix>.info (int32: len, sources, clearance_sq) after the last frame;
 * ground_plan() is also called after every earlier frame.  With max < min it must return false and write nothing into `path`. */
#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc < 14 || (argc - 14) % 2) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known radius frontiers max_len [gx gy]...\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("ground/robot_radius", argv[11]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const bool frontiers = std::stoi(argv[12]) != 0;
        const int max_len = std::stoi(argv[13]);
        std::vector<float> goals;
        for (int i = 14; i < argc; i++) goals.push_back(std::stof(argv[i]));
        gie_host::VolumetricMapper vm(p);
        std::vector<std::array<int32_t, 2>> path(3, std::array<int32_t, 2>{ 0x5a5a5a5a, 0x5a5a5a5a });
        int made = 0;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_plan(goals.data(), (int)goals.size() / 2, frontiers, max_len, path) ? 1 : 0;
        }
        const std::string out = argv[2];
        const int32_t info[3] = { vm.ground_plan_len, vm.ground_plan_sources, vm.ground_clearance_sq() };
        dump(out + ".path", path.data(), path.size() * sizeof(path[0]));
        dump(out + ".info", info, sizeof(info));
        printf("frames %d made %d points %zu\n", in.frames, made, path.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_plan_probe: %s\n", e.what()); return 1; }
    return 0;
}
