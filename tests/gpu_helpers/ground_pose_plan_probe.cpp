/* Test helper (tests/test_ground_pose_nf1_gpu.py): VolumetricMapper::ground_plan_footprint over a few point-cloud frames, the last result as raw files.
 *   ground_pose_plan_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 *                          <footprint: "front back half_width" or "-"> <band: 1, or 0 to leave the band unset> <yaw> <reverse 0|1> <max_len>
 *                          goal_x goal_y goal_yaw [goal_x goal_y goal_yaw]...      (goal_yaw "nan" = any heading)
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * After every frame: ground_plan_footprint() to the goals.  Writes <prefix>.path (the triples of the last call, int32) and <prefix>.info (int32:
 * calls that returned true, ground_pose_plan_len, ground_pose_plan_sources, the start's heading index, front_sq, back_sq, side_sq) after the last
 * frame.  With the footprint or the band unset the call must refuse and leave the path and the two members alone. */
#include <cstring>

#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc < 19 || (argc - 16) % 3) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known footprint band yaw reverse max_len gx gy gyaw [gx gy gyaw]...\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        if (std::stoi(argv[12])) { p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); }
        p.set("ground/min_known", argv[10]);
        if (strcmp(argv[11], "-")) p.set("ground/footprint", argv[11]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const float yaw = std::stof(argv[13]);
        const bool reverse = std::stoi(argv[14]) != 0;
        const int max_len = std::stoi(argv[15]);
        std::vector<float> goals, yaws;
        for (int i = 16; i + 2 < argc; i += 3) { goals.push_back(std::stof(argv[i])); goals.push_back(std::stof(argv[i + 1])); yaws.push_back(std::stof(argv[i + 2])); }
        gie_host::VolumetricMapper vm(p);
        std::vector<std::array<int32_t, 3>> path(2, std::array<int32_t, 3>{ -7, -7, -7 });
        vm.ground_pose_plan_len = -5; vm.ground_pose_plan_sources = -6;
        int made = 0;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_plan_footprint(yaw, goals.data(), yaws.data(), (int)yaws.size(), false, reverse, max_len, path) ? 1 : 0;
        }
        const std::string out = argv[2];
        const std::array<int32_t, 3> sq = vm.ground_footprint_sq();
        const int32_t info[7] = { made, vm.ground_pose_plan_len, vm.ground_pose_plan_sources, gie_host::VolumetricMapper::ground_heading_index((double)yaw), sq[0], sq[1], sq[2] };
        dump(out + ".path", path.data(), path.size() * sizeof(path[0]));
        dump(out + ".info", info, sizeof(info));
        printf("frames %d made %d len %d sources %d triples %zu\n", in.frames, made, vm.ground_pose_plan_len, vm.ground_pose_plan_sources, path.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_pose_plan_probe: %s\n", e.what()); return 1; }
    return 0;
}
