// policy_table.cpp -- the launch policy (csrc/fx_policy.h) on rows of plan steps read from standard input, without a GPU
// (tests/test_launch_policy.py builds it with the compiler's host pass and compares its answers with a recording of real contexts).
//
// in:  per row  name | max_agents max_cand max_steps max_knots max_obs max_pred | G wpe variant block mapping obst_stage obst_CH fused
//               store step_kernel step_kernel_CH | package last_live cap3 cap5 cap8 lds_pad obst_wg | n_agents, then per agent
//               N M K P mode nT nV nD n_rows matrix shard_begin shard_count n_bound have_hull n_cost cost_id...
// out: per row  name lds <per agent: M S rec base generic generic_rec>   the generic kernel's LDS: what must fit (fx_generic_base_lds),
//                        what a launch asks for without and with rec bytes of staged records (fx_generic_lds), rec = fx_rec_lds_bytes
//      then      name ok <16 numbers of fx_step_info_ex> <one-launch step: CH blocks lds>   or   name err <code> <message>
//      then      name launch <M_max S_max gen_rec_lds> <fx_generic_lds of them>   for a row the generic kernel runs
//      at the end, per part list:  #layout <n> <bytes...> <offsets...> <size>   an FxBlockLayout walk (csrc/fx_pass.h)
//      and the two rules of the passes that work in items (csrc/fx_pass.h):
//                #items chunk <n> <S> <K> <forced> <fx_item_chunk_steps>   and   #items batch <per_candidate_bytes> <n> <fx_item_batch>
#include <iostream>
#include <string>
#include <vector>

#include "fx_pass.h"
#include "fx_policy.h"

int main() {
    std::string name;
    static const double some_doubles[1] = {0.0};
    static const int32_t some_ints[1] = {0};
    while (std::cin >> name) {
        long long max_cand;
        int max_agents, max_steps, max_knots, max_obs, max_pred, fused, package, n_agents, cap[3];
        long long last_live, lds_pad;
        FxForce f;
        std::cin >> max_agents >> max_cand >> max_steps >> max_knots >> max_obs >> max_pred;
        std::cin >> f.G >> f.wpe >> f.variant >> f.block >> f.wsplit >> f.obst_stage >> f.obst_CH >> fused >> f.store >> f.step_kernel >>
            f.step_kernel_CH;
        std::cin >> package >> last_live >> cap[0] >> cap[1] >> cap[2] >> lds_pad >> f.obst_wg >> n_agents;
        f.fuse_enabled = fused != 0;
        f.fuse_any_size = fused == 2;
        f.lds_pad = (size_t)lds_pad;
        std::vector<FxProblem> probs(n_agents);
        std::vector<std::vector<int32_t>> ids(n_agents);
        for (int a = 0; a < n_agents; a++) {
            FxProblem &p = probs[a];
            p = FxProblem();
            int matrix, have_hull;
            long long n_rows, shard_begin, shard_count;
            std::cin >> p.N >> p.M >> p.K >> p.P >> p.mode >> p.nT >> p.nV >> p.nD >> n_rows >> matrix >> shard_begin >> shard_count >>
                p.n_bound >> have_hull >> p.n_cost;
            p.n_rows = n_rows; p.shard_begin = shard_begin; p.shard_count = shard_count;
            ids[a].resize(p.n_cost);
            for (int n = 0; n < p.n_cost; n++) std::cin >> ids[a][n];
            p.cost_id = ids[a].data();
            if (matrix) p.sampling_matrix = some_doubles;   // (the policy asks only whether the arrays are there)
            if (have_hull) { p.obs_hull = some_doubles; p.obs_nhull = some_ints; }
        }
        if (!std::cin) { std::cerr << "bad row " << name << "\n"; return 2; }
        std::cout << name << " lds";
        for (const FxProblem &p : probs) {
            const int S = p.N + 1;
            const size_t rec = fx_rec_lds_bytes(true, S, p.K);
            std::cout << " " << p.M << " " << S << " " << rec << " " << fx_generic_base_lds(&p) << " " << fx_generic_lds(p.M, S, 0) << " "
                      << fx_generic_lds(p.M, S, rec);
        }
        std::cout << "\n";
        std::vector<FxAgentPlan> rows(n_agents);
        FxStepPlan pl;
        pl.agents = rows.data();
        char err[512] = "";
        const int rc = fx_plan_upload(n_agents, probs.data(), f, fx_caps_of(max_agents, max_cand, max_steps, max_knots, max_obs, max_pred), &pl,
                                      err, sizeof(err));
        if (rc) { std::cout << name << " err " << rc << " " << err << "\n"; continue; }
        FxLaunchPlan L = fx_plan_launches(pl, f, package != 0);
        FxStepKernelSize sz;
        if (L.try_step_kernel) {
            sz = fx_plan_step_kernel(pl, f, last_live, cap);
            if (sz.CH) fx_take_step_kernel(L, sz);
        }
        int64_t v[16];
        fx_step_info_of(pl, L, 0, v);
        std::cout << name << " ok";
        for (int i = 0; i < 16; i++) std::cout << " " << v[i];
        std::cout << " " << sz.CH << " " << sz.blocks << " " << sz.lds << "\n";
        if (!pl.use_grid)
            std::cout << name << " launch " << pl.M_max << " " << pl.S_max << " " << pl.gen_rec_lds << " "
                      << fx_generic_lds(pl.M_max, pl.S_max, pl.gen_rec_lds) << "\n";
    }
    // the layout of a device block: the sizes either side of the 8-byte floor and of the 256-byte alignment, a large part, none
    const std::vector<std::vector<size_t>> part_lists = {
        {0, 1, 255, 256, 257}, {257, 256, 255, 1, 0}, {8, 7, 9, 511, 512, 513, 0, 0}, {1}, {(size_t)5 << 30, 3, 1000000007}, {}};
    for (const std::vector<size_t> &parts : part_lists) {
        FxBlockLayout lay;
        std::vector<size_t> offs;
        for (size_t b : parts) offs.push_back(lay.take(b));
        std::cout << "#layout " << parts.size();
        for (size_t b : parts) std::cout << " " << b;
        for (size_t o : offs) std::cout << " " << o;
        std::cout << " " << lay.size() << "\n";
    }
    // steps per chunk: the planner's grid and config 3 (as recorded on the device), a forced size beyond the horizon, a horizon of one sample
    const long long chunk_calls[][4] = {{2176, 31, 8, 0}, {50388, 31, 20, 0}, {1, 31, 1, 99},  {2176, 31, 8, 99}, {50388, 31, 20, 99},
                                        {1, 1, 0, 0},     {2176, 1, 8, 0},    {50388, 1, 20, 0}};
    for (const auto &q : chunk_calls)
        std::cout << "#items chunk " << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << " "
                  << fx_item_chunk_steps(q[0], (int)q[1], (int)q[2], (int)q[3]) << "\n";
    // candidates per batch: two batches of the planner's grid, one tile for one candidate and for none, a ragged second tile, a share
    // of a candidate beyond the bound
    const std::pair<size_t, long long> batch_calls[] = {
        {(size_t)7 * 20 * 30 * 8, 2176}, {100, 1}, {100, 0}, {100, 65}, {2 * FX_ITEM_SCRATCH_BYTES, 1000}};
    for (const auto &q : batch_calls) std::cout << "#items batch " << q.first << " " << q.second << " " << fx_item_batch(q.first, q.second) << "\n";
    return 0;
}
