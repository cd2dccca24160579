/* Test helper (tests/test_costmat_host_gpu.py): VolumetricMapper::exploration_costs over a few point-cloud frames, as raw files.
 *   costmat_host_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <max_clusters> <clearance_m> <min_size>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.goals (3 * (max_clusters + 1) float32) and <prefix>.cost ((max_clusters + 1)^2 int32) after the last frame;
 * exploration_costs() is also called after every earlier frame.  Built with -DGIE_HOST_WITH_HIP: the method needs the HIP runtime's headers and library. */
#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc != 11) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff max_clusters clearance min_size\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const int max_clusters = std::stoi(argv[8]), min_size = std::stoi(argv[10]);
        const float clearance = std::stof(argv[9]);
        gie_host::VolumetricMapper vm(p);
        const int frames = in.frames;
        std::vector<int32_t> cost;
        std::vector<float> goals;
        int kept = -1;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            kept = vm.exploration_costs(max_clusters, clearance, min_size, cost, goals);
        }
        const std::string out = argv[2];
        dump(out + ".goals", goals.data(), goals.size() * sizeof(float));
        dump(out + ".cost", cost.data(), cost.size() * sizeof(int32_t));
        printf("frames %d kept %d points %zu\n", frames, kept, goals.size() / 3);
    } catch (const std::exception &e) { fprintf(stderr, "costmat_host_probe: %s\n", e.what()); return 1; }
    return 0;
}
