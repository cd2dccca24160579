/* Test helper (tests/test_ground_footprint_gpu.py): VolumetricMapper::ground_local_plan_footprint over a few point-cloud frames, the last result as raw files.
 *   ground_footprint_plan_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 *                               <robot_radius> <footprint: "front back half_width" or "-"> <yaw> <dt> <T> <inflate_radius> <v_min> <v_max> <omega_max>
 *                               goal_x goal_y [goal_x goal_y]...
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * After every frame: ground_plan() to the goals, ground_local_plan() and ground_local_plan_footprint() with the same 9 x 9 samples (v, omega),
 * v_min .. v_max by -omega_max .. omega_max.  Writes <prefix>.v and <prefix>.omega (81 floats each), <prefix>.poses (81 * T * 2 floats),
 * <prefix>.headings (81 * T * 2 int32), <prefix>.rec (81 records of 48 bytes), <prefix>.fp (81 records of 32 bytes), <prefix>.plain_poses and
 * <prefix>.plain_rec (what ground_local_plan() returned) and <prefix>.info (int32: the index, ground_local_plan()'s index, clearance_sq, front_sq,
 * back_sq, side_sq) after the last frame.  With "-" the footprint stays unset: the call must refuse and write nothing into the four vectors. */
#include <cstring>

#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc < 22 || (argc - 20) % 2) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known radius footprint yaw dt T inflate v_min v_max omega_max gx gy [gx gy]...\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("ground/robot_radius", argv[11]);
        if (strcmp(argv[12], "-")) p.set("ground/footprint", argv[12]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const float yaw = std::stof(argv[13]), dt = std::stof(argv[14]), inflate = std::stof(argv[16]);
        const int T = std::stoi(argv[15]);
        const float v_min = std::stof(argv[17]), v_max = std::stof(argv[18]), omega_max = std::stof(argv[19]);
        std::vector<float> goals;
        for (int i = 20; i < argc; i++) goals.push_back(std::stof(argv[i]));
        std::vector<float> v(81), omega(81);
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) { v[(size_t)i * 9 + j] = v_min + (v_max - v_min) * (float)i / 8.f; omega[(size_t)i * 9 + j] = -omega_max + 2.f * omega_max * (float)j / 8.f; }
        gie_host::VolumetricMapper vm(p);
        gie_ground_rollout poison;
        memset(&poison, 0x5a, sizeof(poison));
        gie_ground_footprint fpoison;
        memset(&fpoison, 0x5a, sizeof(fpoison));
        std::vector<gie_ground_rollout> records(2, poison), plain_records;
        std::vector<gie_ground_footprint> footprints(2, fpoison);
        std::vector<float> poses(3, -7.f), plain_poses;
        std::vector<int32_t> headings(3, -7);
        std::vector<std::array<int32_t, 2>> path;
        int made = 0, best = -1, plain = -1;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_plan(goals.data(), (int)goals.size() / 2, false, 64, path) ? 1 : 0;
            plain = vm.ground_local_plan(yaw, v.data(), omega.data(), 81, dt, T, inflate, plain_poses, plain_records);
            best = vm.ground_local_plan_footprint(yaw, v.data(), omega.data(), 81, dt, T, inflate, poses, headings, records, footprints);
        }
        const std::string out = argv[2];
        const std::array<int32_t, 3> sq = vm.ground_footprint_sq();
        const int32_t info[6] = { best, plain, vm.ground_clearance_sq(), sq[0], sq[1], sq[2] };
        dump(out + ".v", v.data(), v.size() * sizeof(float));
        dump(out + ".omega", omega.data(), omega.size() * sizeof(float));
        dump(out + ".poses", poses.data(), poses.size() * sizeof(float));
        dump(out + ".headings", headings.data(), headings.size() * sizeof(int32_t));
        dump(out + ".rec", records.data(), records.size() * sizeof(records[0]));
        dump(out + ".fp", footprints.data(), footprints.size() * sizeof(footprints[0]));
        dump(out + ".plain_poses", plain_poses.data(), plain_poses.size() * sizeof(float));
        dump(out + ".plain_rec", plain_records.data(), plain_records.size() * sizeof(gie_ground_rollout));
        dump(out + ".info", info, sizeof(info));
        printf("frames %d made %d best %d plain %d poses %zu headings %zu records %zu footprints %zu\n", in.frames, made, best, plain, poses.size(), headings.size(),
               records.size(), footprints.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_footprint_plan_probe: %s\n", e.what()); return 1; }
    return 0;
}
