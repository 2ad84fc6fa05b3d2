// Stand-alone check of the env-step launch plan (csrc/macjd_env_plan.h), built with -fsanitize=address,undefined and run as a
// child process by tests/test_env_plan_cpu.py.  The table restates the expressions the launch functions used before the plan
// became one function: block from n_envs * many_T, x extent of a many-step grid from n_envs alone, strided grid capped at
// 2048 workgroups of 256 lanes.
#include <cstdint>
#include <cstdio>

#include "../ma-cjd-cooperative-jamming-decision-making-via-marl_amd/csrc/macjd_env_plan.h"

struct Row {
    int64_t n_envs;
    int32_t many_T;
    int block;
    int64_t full_x;
    int32_t full_y;
    unsigned strided;
};

static const Row rows[] = {
    {1, 0, 64, 1, 1, 1},           {64, 0, 64, 1, 1, 1},           {65, 0, 64, 2, 1, 2},
    {65535, 0, 64, 1024, 1, 1024}, {65536, 0, 256, 256, 1, 256},   {300000, 0, 256, 1172, 1, 1172},
    {600000, 0, 256, 2344, 1, 2048}, {100, 3, 64, 2, 3, 5},        {30000, 3, 256, 118, 3, 352},
};

int main() {
    int bad = 0;
    for (const Row& r : rows) {
        const macjd::LanePlan p = macjd::lane_plan(r.n_envs, r.many_T);
        const int64_t items = r.n_envs * (r.many_T > 0 ? r.many_T : 1);
        const bool ok = p.block == r.block && p.full_x == r.full_x && p.full_y == r.full_y && p.strided == r.strided &&
                        p.blocks == (items + r.block - 1) / r.block;
        std::printf("%s n_envs=%lld many_T=%d: block %d full (%lld, %d) strided %u blocks %lld\n", ok ? "ok  " : "FAIL",
                    (long long)r.n_envs, (int)r.many_T, p.block, (long long)p.full_x, (int)p.full_y, p.strided, (long long)p.blocks);
        bad += !ok;
    }
    // every item of a full grid has a lane; the strided grid never exceeds the full one's workgroups
    for (int64_t n = 1; n <= 700000; n += 997)
        for (int32_t T = 0; T <= 3; T += 3) {
            const macjd::LanePlan p = macjd::lane_plan(n, T);
            const bool ok = p.full_x * p.block >= n && p.full_y == (T > 0 ? T : 1) && p.strided >= 1 && (int64_t)p.strided <= p.blocks;
            if (!ok) { std::printf("FAIL n_envs=%lld many_T=%d\n", (long long)n, (int)T); ++bad; }
        }
    std::printf(bad ? "failed: %d\n" : "ok: %d rows\n", bad ? bad : (int)(sizeof(rows) / sizeof(rows[0])));
    return bad ? 1 : 0;
}
