/* Test helper (tests/test_routes_gpu.py): VolumetricMapper::global_frontier_routes over a few point-cloud frames, the goals printed.
 *   routes_host_probe <frames.f32> <voxel_width> <X> <Y> <Z> <cutoff_dist> <min_fnt> <max_goals> <route_min_free> <route_min_open>
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * The three thresholds go through the parameters explore/min_fnt, explore/route_min_free and explore/route_min_open.  Prints
 * "blocks <n> goals <k>", then one line per goal: the bit patterns of its position's three floats (hex), its key, n_fnt,
 * min_dist_sq and steps. */
#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc != 11) { fprintf(stderr, "usage: %s frames voxel X Y Z cutoff min_fnt max_goals route_min_free route_min_open\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[2], argv[3], argv[4], argv[5], argv[6]);
        p.set("cpu_mirror", "false");
        p.set("explore/min_fnt", argv[7]);
        p.set("explore/route_min_free", argv[9]);
        p.set("explore/route_min_open", argv[10]);
        gie_host::VolumetricMapper vm(p);
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) vm.publishMap(pose, f);
        std::vector<gie_host::FrontierRouteGoal> goals;
        const int n = vm.global_frontier_routes(std::stoi(argv[8]), goals);
        printf("blocks %d goals %zu\n", n, goals.size());
        for (const gie_host::FrontierRouteGoal &g : goals) {
            uint32_t b[3];
            std::memcpy(b, g.pos, 12);
            printf("%08x %08x %08x %d %d %d %d %d %d\n", b[0], b[1], b[2], g.key[0], g.key[1], g.key[2], g.n_fnt, g.min_dist_sq, g.steps);
        }
    } catch (const std::exception &e) { fprintf(stderr, "routes_host_probe: %s\n", e.what()); return 1; }
    return 0;
}
