/* Test helper (tests/test_cloud_gpu.py): VolumetricMapper::visualize over a few point-cloud frames, the four clouds as raw files.
 *   cloud_host_probe <frames.f32> <out prefix> <cpu_mirror 0|1> <voxel_width> <X> <Y> <Z> <cutoff_dist> <vis_height>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.loc_ogm / .loc_edt / .glb_ogm / .glb_edt (gie_cloud_point records) after the last frame; visualize() is also
 * called after every earlier frame, as the reference does with vis_interval 1. */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "../../gie-mapping_amd/host/gie_host.hpp"

static void dump(const std::string &path, const std::vector<gie_cloud_point> &c)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.data()), (std::streamsize)(c.size() * sizeof(gie_cloud_point)));
    if (!f) throw std::runtime_error("cannot write " + path);
}

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: %s frames out cpu_mirror voxel X Y Z cutoff vis_height\n", argv[0]); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) throw std::runtime_error("cannot open the frames");
        const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const float *w = reinterpret_cast<const float *>(raw.data());
        const size_t nw = raw.size() / sizeof(float);
        gie_host::Parameters p;
        const float voxel = std::stof(argv[4]);
        p.set("cpu_mirror", argv[3]);
        p.set("voxel_width", argv[4]);
        p.set("local_size_x", std::to_string(std::stoi(argv[5]) * voxel + 1e-4f));
        p.set("local_size_y", std::to_string(std::stoi(argv[6]) * voxel + 1e-4f));
        p.set("local_size_z", std::to_string(std::stoi(argv[7]) * voxel + 1e-4f));
        p.set("wave/cutoff_dist", argv[8]);
        p.set("vis_height", argv[9]);
        p.set("wave/fast_mode", "false");
        p.set("ogm/min_height", "-1000"); p.set("ogm/max_height", "1000");
        for (const char *k : { "display_loc_ogm", "display_loc_edt", "display_glb_ogm", "display_glb_edt" }) p.set(k, "true");
        gie_host::VolumetricMapper vm(p);
        if (nw < 1) throw std::runtime_error("empty frames file");
        const int frames = (int)w[0];
        size_t at = 1;
        const float sensor[3] = { 0.f, 0.f, 0.f };
        for (int k = 0; k < frames; k++) {
            if (at + 8 > nw) throw std::runtime_error("truncated frames file");
            gie_host::Pose pose;
            for (int i = 0; i < 3; i++) pose.pos[i] = w[at + i];
            for (int i = 0; i < 4; i++) pose.quat_wxyz[i] = w[at + 3 + i];
            const int n = (int)w[at + 7];
            at += 8;
            if (n < 0 || at + 3 * (size_t)n > nw) throw std::runtime_error("truncated frames file");
            gie_host::VolumetricMapper::Frame f = {};
            f.kind = gie_host::VolumetricMapper::POINTCLOUD; f.data = w + at; f.n = n;
            at += 3 * (size_t)n;
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
