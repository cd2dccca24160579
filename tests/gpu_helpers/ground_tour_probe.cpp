/* Test helper (tests/test_ground_costmat_gpu.py): VolumetricMapper::ground_exploration_costs over a few point-cloud frames, the last
 * result as raw files.
 *   ground_tour_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 *                     <robot_radius> <max_clusters> <min_size>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.cost (int32, (max_clusters + 1)^2), <prefix>.goals (float32, 2 * (max_clusters + 1)) and <prefix>.info (int32: kept,
 * cells, clearance_sq) after the last frame; ground_exploration_costs() is also called after every earlier frame.  With max < min it
 * must return false and write nothing into the two vectors.  Built with -DGIE_HOST_WITH_HIP: the method needs the HIP runtime's
 * headers and library. */
#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc != 14) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known radius max_clusters min_size\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("ground/robot_radius", argv[11]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const int max_clusters = std::stoi(argv[12]), min_size = std::stoi(argv[13]);
        gie_host::VolumetricMapper vm(p);
        std::vector<int32_t> cost(3, 0x5a5a5a5a);
        std::vector<float> goals(2, -7.f);
        int made = 0;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_exploration_costs(max_clusters, min_size, cost, goals) ? 1 : 0;
        }
        const std::string out = argv[2];
        const int32_t info[3] = { vm.ground_goals_kept, vm.ground_goals_cells, vm.ground_clearance_sq() };
        dump(out + ".cost", cost.data(), cost.size() * sizeof(cost[0]));
        dump(out + ".goals", goals.data(), goals.size() * sizeof(goals[0]));
        dump(out + ".info", info, sizeof(info));
        printf("frames %d made %d cost %zu goals %zu\n", in.frames, made, cost.size(), goals.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_tour_probe: %s\n", e.what()); return 1; }
    return 0;
}
