/* Test helper (tests/test_costmat_host_gpu.py): VolumetricMapper::exploration_costs over a few point-cloud frames, as raw files.
 *   costmat_host_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <max_clusters> <clearance_m> <min_size>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * Writes <prefix>.goals (3 * (max_clusters + 1) float32) and <prefix>.cost ((max_clusters + 1)^2 int32) after the last frame;
 * exploration_costs() is also called after every earlier frame.  Built with -DGIE_HOST_WITH_HIP: the method needs the HIP runtime's headers and library. */
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
    if (argc != 11) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff max_clusters clearance min_size\n", argv[0]); return 2; }
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
        p.set("wave/fast_mode", "false");
        p.set("ogm/min_height", "-1000"); p.set("ogm/max_height", "1000");
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const int max_clusters = std::stoi(argv[8]), min_size = std::stoi(argv[10]);
        const float clearance = std::stof(argv[9]);
        gie_host::VolumetricMapper vm(p);
        if (nw < 1) throw std::runtime_error("empty frames file");
        const int frames = (int)w[0];
        size_t at = 1;
        std::vector<int32_t> cost;
        std::vector<float> goals;
        int kept = -1;
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
            kept = vm.exploration_costs(max_clusters, clearance, min_size, cost, goals);
        }
        const std::string out = argv[2];
        dump(out + ".goals", goals.data(), goals.size() * sizeof(float));
        dump(out + ".cost", cost.data(), cost.size() * sizeof(int32_t));
        printf("frames %d kept %d points %zu\n", frames, kept, goals.size() / 3);
    } catch (const std::exception &e) { fprintf(stderr, "costmat_host_probe: %s\n", e.what()); return 1; }
    return 0;
}
