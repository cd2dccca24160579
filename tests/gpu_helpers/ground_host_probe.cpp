/* Test helper (tests/test_ground_gpu.py): VolumetricMapper::ground_costmap over a few point-cloud frames, the last CostMap as raw files.
 *   ground_host_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.payload (gie_seendist), <prefix>.hdr (gie_costmap_hdr) and <prefix>.counts (4 int32) after the last frame;
 * ground_costmap() is also called after every earlier frame.  With max < min it must return false and write nothing. */
#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc != 11) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        gie_host::VolumetricMapper vm(p);
        const int frames = in.frames;
        std::vector<gie_seendist> payload;
        gie_costmap_hdr hdr;
        std::memset(&hdr, 0x5a, sizeof(hdr));
        int made = 0;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_costmap(payload, hdr) ? 1 : 0;
        }
        const std::string out = argv[2];
        dump(out + ".payload", payload.data(), payload.size() * sizeof(gie_seendist));
        dump(out + ".hdr", &hdr, sizeof(hdr));
        dump(out + ".counts", vm.ground_counts, sizeof(vm.ground_counts));
        printf("frames %d made %d cells %zu\n", frames, made, payload.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_host_probe: %s\n", e.what()); return 1; }
    return 0;
}
