/* Test helper (tests/test_ground_rollout_gpu.py): VolumetricMapper::ground_local_plan over a few point-cloud frames, the last result as raw files.
 *   ground_local_plan_probe <frames.f32> <out prefix> <voxel_width> <X> <Y> <Z> <cutoff_dist> <ground_min_height> <ground_max_height> <min_known>
 *                           <robot_radius> <yaw> <dt> <T> <inflate_radius> <v_min> <v_max> <omega_max> goal_x goal_y [goal_x goal_y]...
 * frames.f32: float32 words — the number of frames, then per frame pos[3], quat_wxyz[4], n, n * 3 coordinates (sensor frame).
 * After every frame: ground_plan() to the goals, then ground_local_plan() with 9 x 9 samples (v, omega), v_min .. v_max by -omega_max ..
 * omega_max.  Writes <prefix>.v and <prefix>.omega (81 floats each), <prefix>.poses (81 * T * 2 floats), <prefix>.rec (81 records of 48
 * bytes) and <prefix>.info (int32: the index, clearance_sq) after the last frame.  With max < min both calls must refuse and write
 * nothing into the two vectors. */
#include <cstring>

#include "host_probe.hpp"

int main(int argc, char **argv)
{
    if (argc < 21 || (argc - 19) % 2) { fprintf(stderr, "usage: %s frames out voxel X Y Z cutoff ground_min ground_max min_known radius yaw dt T inflate v_min v_max omega_max gx gy [gx gy]...\n", argv[0]); return 2; }
    try {
        FramesFile in(argv[1]);
        gie_host::Parameters p = probe_parameters(argv[3], argv[4], argv[5], argv[6], argv[7]);
        p.set("ground/min_height", argv[8]); p.set("ground/max_height", argv[9]); p.set("ground/min_known", argv[10]);
        p.set("ground/robot_radius", argv[11]);
        p.set("display_glb_edt", "false"); p.set("display_glb_ogm", "false");
        const float yaw = std::stof(argv[12]), dt = std::stof(argv[13]), inflate = std::stof(argv[15]);
        const int T = std::stoi(argv[14]);
        const float v_min = std::stof(argv[16]), v_max = std::stof(argv[17]), omega_max = std::stof(argv[18]);
        std::vector<float> goals;
        for (int i = 19; i < argc; i++) goals.push_back(std::stof(argv[i]));
        std::vector<float> v(81), omega(81);
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) { v[(size_t)i * 9 + j] = v_min + (v_max - v_min) * (float)i / 8.f; omega[(size_t)i * 9 + j] = -omega_max + 2.f * omega_max * (float)j / 8.f; }
        gie_host::VolumetricMapper vm(p);
        gie_ground_rollout poison;
        memset(&poison, 0x5a, sizeof(poison));
        std::vector<gie_ground_rollout> records(2, poison);
        std::vector<float> poses(3, -7.f);
        std::vector<std::array<int32_t, 2>> path;
        int made = 0, best = -1;
        gie_host::Pose pose;
        gie_host::VolumetricMapper::Frame f;
        while (in.next(pose, f)) {
            vm.publishMap(pose, f);
            made += vm.ground_plan(goals.data(), (int)goals.size() / 2, false, 64, path) ? 1 : 0;
            best = vm.ground_local_plan(yaw, v.data(), omega.data(), 81, dt, T, inflate, poses, records);
        }
        const std::string out = argv[2];
        const int32_t info[2] = { best, vm.ground_clearance_sq() };
        dump(out + ".v", v.data(), v.size() * sizeof(float));
        dump(out + ".omega", omega.data(), omega.size() * sizeof(float));
        dump(out + ".poses", poses.data(), poses.size() * sizeof(float));
        dump(out + ".rec", records.data(), records.size() * sizeof(records[0]));
        dump(out + ".info", info, sizeof(info));
        printf("frames %d made %d best %d poses %zu records %zu\n", in.frames, made, best, poses.size(), records.size());
    } catch (const std::exception &e) { fprintf(stderr, "ground_local_plan_probe: %s\n", e.what()); return 1; }
    return 0;
}
