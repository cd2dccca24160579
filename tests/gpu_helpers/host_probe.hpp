/* What the host-layer probes (cloud_host_probe.cpp, ground_host_probe.cpp, costmat_host_probe.cpp) share: raw output files, the
 * parameters of the VolumetricMapper they all set, and the reader of frames.f32.
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame). */
#pragma once
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

/* a local volume of X x Y x Z voxels, the exact waves, no height limits on the occupancy */
static gie_host::Parameters probe_parameters(const char *voxel_width, const char *X, const char *Y, const char *Z, const char *cutoff_dist)
{
    gie_host::Parameters p;
    const float voxel = std::stof(voxel_width);
    p.set("voxel_width", voxel_width);
    p.set("local_size_x", std::to_string(std::stoi(X) * voxel + 1e-4f));
    p.set("local_size_y", std::to_string(std::stoi(Y) * voxel + 1e-4f));
    p.set("local_size_z", std::to_string(std::stoi(Z) * voxel + 1e-4f));
    p.set("wave/cutoff_dist", cutoff_dist);
    p.set("wave/fast_mode", "false");
    p.set("ogm/min_height", "-1000"); p.set("ogm/max_height", "1000");
    return p;
}

/* the frames of a frames.f32, one after the other; the points of a Frame stay in the file's buffer */
struct FramesFile {
    std::vector<char> raw;
    const float *w;
    size_t nw, at = 1;
    int frames, k = 0;

    explicit FramesFile(const char *path)
    {
        std::ifstream in(path, std::ios::binary);
        if (!in) throw std::runtime_error("cannot open the frames");
        raw.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        w = reinterpret_cast<const float *>(raw.data());
        nw = raw.size() / sizeof(float);
        if (nw < 1) throw std::runtime_error("empty frames file");
        frames = (int)w[0];
    }

    static void whole(bool ok) { if (!ok) throw std::runtime_error("truncated frames file"); }

    bool next(gie_host::Pose &pose, gie_host::VolumetricMapper::Frame &f)
    {
        if (k++ >= frames) return false;
        whole(at + 8 <= nw);
        for (int i = 0; i < 3; i++) pose.pos[i] = w[at + i];
        for (int i = 0; i < 4; i++) pose.quat_wxyz[i] = w[at + 3 + i];
        const int n = (int)w[at + 7];
        at += 8;
        whole(n >= 0 && at + 3 * (size_t)n <= nw);
        f = {};
        f.kind = gie_host::VolumetricMapper::POINTCLOUD; f.data = w + at; f.n = n;
        at += 3 * (size_t)n;
        return true;
    }
};
