/* Test helper (tests/test_cloud_gpu.py): VolumetricMapper::visualize over a few point-cloud frames, the four clouds as raw files.
 *   cloud_host_probe <frames.f32> <out prefix> <cpu_mirror 0|1> <voxel_width> <X> <Y> <Z> <cutoff_dist> <vis_height>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.loc_ogm / .loc_edt / .glb_ogm / .glb_edt (gie_cloud_point records) after the last frame; visualize() is also
 * called after every earlier frame, as the reference does with vis_interval 1. */
#include "host_probe.hpp"

static void dump(const std::string &path, const std::vector<gie_cloud_point> &c) { dump(path, c.data(), c.size() * sizeof(gie_cloud_point)); }

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: %s frames out cpu_mirror voxel X Y Z cutoff vis_height\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[4], argv[5], argv[6], argv[7], argv[8]);
        p.set("cpu_mirror", argv[3]);
        p.set("vis_height", argv[9]);
        for (const char *k : { "display_loc_ogm", "display_loc_edt", "display_glb_ogm", "display_glb_edt" }) p.set(k, "true");
        gie_host::VolumetricMapper vm(p);
        const int frames = in.frames;
        const float sensor[3] = { 0.f, 0.f, 0.f };
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            vm.visualize(sensor);
        }
        const gie_host::DisplayClouds &c = vm.clouds;
        const std::string out = argv[2];
        dump(out + ".loc_ogm", c.loc_ogm); dump(out + ".loc_edt", c.loc_edt); dump(out + ".glb_ogm", c.glb_ogm); dump(out + ".glb_edt", c.glb_edt);
        printf("frames %d streamed %d mirror_blocks %zu loc_ogm %zu loc_edt %zu glb_ogm %zu glb_edt %zu\n", frames, vm.streamed_blocks,
               vm.mirror.block_keys.size(), c.loc_ogm.size(), c.loc_edt.size(), c.glb_ogm.size(), c.glb_edt.size());
    } catch (const std::exception &e) { fprintf(stderr, "cloud_host_probe: %s\n", e.what()); return 1; }
    return 0;
}
