// fx_launch.h -- what fx_kernels.hip defines for the host files (fx_api*.hip), each declared ONCE with its true prototype, and the
// list of their names.  fx_kernels.hip includes this header too, so the compiler holds every definition to its declaration.  A new
// launcher is one declaration and one name in FX_LAUNCHERS: fx_host_stubs.cpp makes the host-only builds' stubs from the list.
// What each launcher does is said at its definition.
#pragma once

#include "fx_device.h"
#include "fx_hypotheses_batch_plan.h"
#include "fx_hypotheses_plan.h"
#include "fx_rescore_batch_plan.h"
#include "fx_rescore_plan.h"
#include "fx_risk_args.h"

struct FxItemRound;   // (fx_pass.h: the host's account of a round of a batched pass)

#define FX_LAUNCHERS(X)                                                                                                          \
    X(fx_launch_eval) X(fx_launch_eval_grid) X(fx_launch_obstacle) X(fx_step_kernel_capacity) X(fx_launch_step) X(fx_launch_select) \
    X(fx_launch_math_test) X(fx_launch_selftest) X(fx_launch_publish) X(fx_launch_stage) X(fx_launch_probe_read) X(fx_launch_package) \
    X(fx_launch_topk) X(fx_launch_gather_candidates) X(fx_launch_eval_list) X(fx_launch_sort) X(fx_launch_sort_gather)               \
    X(fx_launch_risk) X(fx_launch_predprob) X(fx_launch_predprob_batch) X(fx_launch_risk_batch) X(fx_launch_risk_list_batch)         \
    X(fx_launch_risk_costs_batch) X(fx_launch_rescore) X(fx_launch_rescore_batch) X(fx_launch_hypotheses) \
    X(fx_launch_hypotheses_batch)

extern "C" {

hipError_t fx_launch_eval(const DevProblem *d_probs, int n_agents, int max_blocks, size_t lds_bytes, int G, bool bundle, bool obst,
                          bool extra, int wpe, hipEvent_t ev_start, hipEvent_t ev_stop, FuseArgs fuse, hipStream_t stream);
hipError_t fx_launch_eval_grid(const DevProblem *d_probs, int n_agents, int max_blocks, int block_size, size_t lds_bytes, int G,
                               bool bundle, bool obst, int wpe, bool wsplit, hipEvent_t ev_start, hipEvent_t ev_stop, FuseArgs fuse,
                               hipStream_t stream);
hipError_t fx_launch_obstacle(const DevProblem *d_probs, int n_agents, int max_items, size_t lds_bytes, int CH, hipEvent_t ev_start,
                              hipEvent_t ev_stop, hipStream_t stream, int wg_waves, int max_tiles, const DevProblem *head);
hipError_t fx_step_kernel_capacity(int CH, size_t lds_bytes, int *blocks_out);
hipError_t fx_launch_step(const DevProblem *d_probs, int n_agents, int blocks, size_t lds_bytes, int CH, hipEvent_t ev_start,
                          hipEvent_t ev_stop, FuseArgs fuse, StepArgs sa, hipStream_t stream);
hipError_t fx_launch_select(const DevProblem *d_probs, int n_agents, int64_t max_candidates, unsigned long long *host_result,
                            unsigned long long seq, double *dev_winner, double *host_pkg, int pkg_stride, int pkg_plane_rows,
                            hipStream_t stream, const DevProblem *head);
hipError_t fx_launch_math_test(int n, const double *x, double *at, double *sn, double *cs, hipStream_t stream);
hipError_t fx_launch_selftest(int op, int n, const SelftestArgs *args, hipStream_t stream);
hipError_t fx_launch_publish(const double *src, int n, double *host_dst, unsigned long long *host_seq, unsigned long long seq,
                             hipStream_t stream);
hipError_t fx_launch_stage(const void *src_mapped, void *dst, size_t bytes, hipStream_t stream);
hipError_t fx_launch_probe_read(const void *src, void *dst, int blocks, hipStream_t stream);
hipError_t fx_launch_package(const DevProblem *d_probs, int n_agents, const double *winner, double *host_pkg, int stride, int plane_rows,
                             unsigned long long seq, hipStream_t stream);
hipError_t fx_launch_topk(const DevProblem *d_probs, int n_agents, int64_t max_candidates, int k, double *scr_cost, long long *scr_idx,
                          double *out_cost, long long *out_idx, hipStream_t stream);
hipError_t fx_launch_gather_candidates(const GatherArgs *args, const int64_t *d_ids, int64_t n, unsigned long long *d_out,
                                       hipStream_t stream);
hipError_t fx_launch_eval_list(const DevProblem *d_prob, const int64_t *d_ids, int64_t n, size_t lds_bytes, bool obst, bool extra,
                               const EvalListRow *d_rows, int n_rows, int lanes, hipEvent_t ev_start, hipEvent_t ev_stop,
                               hipStream_t stream);
hipError_t fx_launch_sort(const FxSortArgs *args, int n_agents, int64_t max_C, hipEvent_t ev_start, hipEvent_t ev_stop,
                          hipStream_t stream);
hipError_t fx_launch_sort_gather(const int64_t *d_order, int64_t n, const double *cost, const uint32_t *flags, int64_t C,
                                 unsigned long long *out_cost, uint32_t *out_flags, hipStream_t stream);
hipError_t fx_launch_risk(const RiskWalkArgs *walk, const RiskItemArgs *items, double *out_ego, double *out_obst, double *col,
                          double *out_occ, const RiskCostArgs *cost, long long *out_idx, hipEvent_t ev_start, hipEvent_t ev_stop,
                          hipStream_t stream, const RespSumArgs *resp, long long *resp_idx);
hipError_t fx_launch_predprob(const PredProbArgs *args, long long *out_idx, hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream);
hipError_t fx_launch_predprob_batch(const PredProbBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *out_idx,
                                    hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream);
hipError_t fx_launch_risk_batch(const RiskBatchArgs *a, const FxItemRound *rounds, int n_rounds, long long *out_idx, hipEvent_t ev_start,
                                hipEvent_t ev_stop, hipStream_t stream);
hipError_t fx_launch_risk_list_batch(const RiskListBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *out_idx,
                                     hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream);
hipError_t fx_launch_risk_costs_batch(const RiskCostBatchArgs *a, const FxItemRound *rounds, int n_rounds, long long *out_idx,
                                      long long *cost_idx, hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream);
hipError_t fx_launch_rescore(const FxRescoreArgs *a, const FxRescorePlan *p, hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream);
hipError_t fx_launch_rescore_batch(const FxRescoreBatchArgs *a, hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream);
hipError_t fx_launch_hypotheses(const FxHypArgs *a, size_t lds_bytes, hipStream_t stream);
hipError_t fx_launch_hypotheses_batch(const FxHypBatchArgs *a, hipStream_t stream);

// The other way round: host code (fx_api_risk.hip) that fx_launch_predprob calls -- the steps per chunk of its items, the rule of
// fx_pass.h or what a test forces.  No launcher, so not in the list: every host-only build links its definition.
int32_t fx_predprob_chunk_steps(int64_t n, int32_t S, int32_t K);

}  // extern "C"
