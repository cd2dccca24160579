/* Test helper (tests/test_ground_gpu.py): VolumetricMapper::ground_costmap over a few point-cloud frames, the last CostMap as raw files.
 *   ground_host_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.payload (gie_seendist), <prefix>.hdr (gie_costmap_hdr) and <prefix>.counts (4 int32) after the last frame;
 * ground_costmap() is also called after every earlier frame.  With max < min it must return false and write nothing. */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "../../gie-mapping_amd/host/gie_host.hpp"

static void dump(const std::string &path, const void *p, size_t bytes)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(p), (std::streamsize)bytes);
    if (!f) throw std::runtime_error("cannot write " + path);
}

int main(int argc, char **argv)
{
    if (argc != 11) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known\n", argv[0]); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) throw std::runtime_error("cannot open the frames");
        const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const float *w = reinterpret_cast<const float *>(raw.data());
        const size_t nw = raw.size() / sizeof(float);
        gie_host::Parameters p;
        const float voxel = std::stof(argv[3]);
        p.set("voxel_width", argv[3]);
        p.set("local_size_x", std::to_string(std::stoi(argv[4]) * voxel + 1e-4f));
        p.set("local_size_y", std::to_string(std::stoi(argv[5]) * voxel + 1e-4f));
        p.set("local_size_z", std::to_string(std::stoi(argv[6]) * voxel + 1e-4f));
        p.set("wave/cutoff_dist", argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("wave/fast_mode", "false");
        p.set("ogm/min_height", "-1000"); p.set("ogm/max_height", "1000");
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        gie_host::VolumetricMapper vm(p);
        if (nw < 1) throw std::runtime_error("empty frames file");
        const int frames = (int)w[0];
        size_t at = 1;
        std::vector<gie_seendist> payload;
        gie_costmap_hdr hdr;
        std::memset(&hdr, 0x5a, sizeof(hdr));
        int made = 0;
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
