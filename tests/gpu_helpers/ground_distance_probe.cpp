/* Test helper (tests/test_ground_sdf_gpu.py): VolumetricMapper::ground_distance over a few point-cloud frames, the results as raw files.
 *   ground_distance_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known> <points.f32>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * points.f32: float32 words, two per point (metres, world frame).
 * After the last frame: ground_costmap(), then ground_distance() at the points.  Writes <prefix>.dist (float32 per point) and
 * <prefix>.grad (two per point); with max < min both calls must return false and leave their arguments alone. */
#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc != 12) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known points\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        std::ifstream pf(argv[11], std::ios::binary);
        if (!pf) throw std::runtime_error("cannot open the points");
        std::vector<char> raw((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
        const int n = (int)(raw.size() / (2 * sizeof(float)));
        gie_host::VolumetricMapper vm(p);
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) vm.publishMap(pose, f);
        std::vector<gie_seendist> payload;
        gie_costmap_hdr hdr;
        const bool made = vm.ground_costmap(payload, hdr);
        std::vector<float> dist(3, -7.f), grad(5, -7.f);
        const bool ok = vm.ground_distance(reinterpret_cast<const float *>(raw.data()), n, dist, grad);
        const std::string out = argv[2];
        dump(out + ".dist", dist.data(), dist.size() * sizeof(float));
        dump(out + ".grad", grad.data(), grad.size() * sizeof(float));
        printf("made %d ok %d points %d dist %zu grad %zu\n", (int)made, (int)ok, n, dist.size(), grad.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_distance_probe: %s\n", e.what()); return 1; }
    return 0;
}
