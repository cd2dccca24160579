/* Test helper (tests/test_ground_view_gpu.py): VolumetricMapper::ground_exploration_gains over a few point-cloud frames, the last
 * result as raw files.
 *   ground_gains_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 *                      <robot_radius> <max_clusters> <min_size> <r_min> <r_max>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.rec (the records, 64 bytes each), <prefix>.steps (int32 per record), <prefix>.scores (16 bytes per record) and
 * <prefix>.info (int32: kept, cells, clearance_sq) after the last frame; ground_exploration_gains() is also called after every earlier
 * frame.  With max < min it must return false and write nothing into the three vectors.  Built with -DGIE_HOST_WITH_HIP: the method
 * needs the HIP runtime's headers and library. */
#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc != 16) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known radius max_clusters min_size r_min r_max\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("ground/robot_radius", argv[11]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const int max_clusters = std::stoi(argv[12]), min_size = std::stoi(argv[13]);
        const float r_min = std::stof(argv[14]), r_max = std::stof(argv[15]);
        gie_host::VolumetricMapper vm(p);
        gie_ground_frontier_cluster poison;
        memset(&poison, 0x5a, sizeof(poison));
        gie_view_score spoison;
        memset(&spoison, 0x5a, sizeof(spoison));
        std::vector<gie_ground_frontier_cluster> clusters(2, poison);
        std::vector<int32_t> steps(3, 0x5a5a5a5a);
        std::vector<gie_view_score> scores(4, spoison);
        int made = 0;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_exploration_gains(max_clusters, min_size, r_min, r_max, clusters, steps, scores) ? 1 : 0;
        }
        const std::string out = argv[2];
        const int32_t info[3] = { vm.ground_goals_kept, vm.ground_goals_cells, vm.ground_clearance_sq() };
        dump(out + ".rec", clusters.data(), clusters.size() * sizeof(clusters[0]));
        dump(out + ".steps", steps.data(), steps.size() * sizeof(steps[0]));
        dump(out + ".scores", scores.data(), scores.size() * sizeof(scores[0]));
        dump(out + ".info", info, sizeof(info));
        printf("frames %d made %d clusters %zu steps %zu scores %zu\n", in.frames, made, clusters.size(), steps.size(), scores.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_gains_probe: %s\n", e.what()); return 1; }
    return 0;
}
