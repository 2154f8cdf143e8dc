// pairre_host_check.cpp - the host-side argument checks of the PairRE paths (include/kge_hip.h, KGE_PAIRRE), exercised without a GPU:
// every call below is refused before any launch, so the program runs on a machine with no device.  Meant for a sanitizer build of
// the library's HOST code, as a program of its own (nothing is loaded into another process):
//   cd dgl-ke_amd/csrc && for f in *.hip; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined \
//       -c $f -o /tmp/san_${f%.hip}.o; done
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/san_*.o ../../tools/pairre_host_check.cpp -o /tmp/pairre_host_check
//   /tmp/pairre_host_check        (prints "pairre_host_check: N checks passed"; any sanitizer report is a failure)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/kge_hip.h"

static int n_checks = 0;
#define EXPECT(cond)                                                                                       \
    do {                                                                                                   \
        ++n_checks;                                                                                        \
        if (!(cond)) { fprintf(stderr, "line %d: %s  [last error: %s]\n", __LINE__, #cond, kge_last_error()); exit(1); } \
    } while (0)
static bool says(const char *w) { return strstr(kge_last_error(), w) != nullptr; }

int main() {
    float one[4] = {0, 0, 0, 0};                  // a non-null pointer that is never dereferenced by a refused call
    int64_t ids[4] = {0, 0, 0, 0};
    int32_t ranks[4];
    void *p = one;
    EXPECT(kge_abi_version() == 8);
    // widths
    EXPECT(kge_score_pos(KGE_PAIRRE, one, one, one, 2, 8, 8, 1.f, 1.f, one, nullptr) == KGE_ERR_ARG && says("PairRE"));
    EXPECT(kge_score_pos(KGE_PAIRRE, one, one, one, 2, 0, 0, 1.f, 1.f, one, nullptr) == KGE_ERR_ARG && says("PairRE"));
    EXPECT(kge_score_pos(9, one, one, one, 2, 8, 16, 1.f, 1.f, one, nullptr) == KGE_ERR_ARG && says("unknown model"));
    EXPECT(kge_score_pos(KGE_PAIRRE, nullptr, one, one, 2, 8, 16, 1.f, 1.f, one, nullptr) == KGE_ERR_ARG && !says("PairRE"));
    // workspaces one byte short
    size_t need = kge_score_neg_workspace_bytes(KGE_PAIRRE, 2, 8, 24, 32);
    EXPECT(need > kge_score_neg_workspace_bytes(KGE_DISTMULT, 2, 8, 24, 32));
    EXPECT(kge_score_neg_fwd(KGE_PAIRRE, 0, one, one, one, 2, 8, 24, 32, 64, 1.f, 1.f, one, p, need - 1, 0, nullptr) == KGE_ERR_WORKSPACE);
    EXPECT(kge_score_neg_bwd(KGE_PAIRRE, 1, one, one, one, nullptr, one, 2, 8, 24, 32, 64, 1.f, 1.f, one, one, one, p, need - 1, 0, nullptr) ==
           KGE_ERR_WORKSPACE);
    need = kge_rank_workspace_bytes(4, 10, 8);
    EXPECT(kge_rank_eval(KGE_PAIRRE, 0, one, 10, one, 3, ids, ids, ids, 4, 8, 16, 1.f, 1.f, nullptr, 0, nullptr, nullptr, 4, ranks, nullptr, p,
                         need - 1, 0, nullptr) == KGE_ERR_WORKSPACE);
    need = kge_rank_chunked_workspace_bytes(KGE_PAIRRE, 4, 4, 10, 1, 8, 16);
    EXPECT(need > kge_rank_chunked_workspace_bytes(KGE_DISTMULT, 4, 4, 10, 1, 8, 8));
    EXPECT(kge_rank_eval_chunked(KGE_PAIRRE, 0, one, 10, one, 3, nullptr, ids, ids, ids, 8, 8, 16, 1.f, 1.f, 4, nullptr, 0, 0, 1, nullptr,
                                 nullptr, ranks, nullptr, p, need - 1, 0, nullptr) == KGE_ERR_WORKSPACE);
    need = kge_topk_workspace_bytes(64, 10, 2 * 32, 3);
    EXPECT(need > kge_topk_workspace_bytes(64, 10, 32, 3));
    EXPECT(kge_topk_select(KGE_PAIRRE, 0, one, 10, one, 3, ids, ids, ids, 64, 32, 64, 0.f, 1.f, ids, 10, ids, 1, 1, 3, one, ids, p, need - 1,
                           nullptr) == KGE_ERR_WORKSPACE);
    EXPECT(kge_topk_select(KGE_PAIRRE, 0, one, 10, one, 3, ids, ids, ids, 64, 32, 32, 0.f, 1.f, ids, 10, ids, 1, 1, 3, one, ids, p, need,
                           nullptr) == KGE_ERR_ARG && says("do not fit model 10"));
    // the step: size, workspace, the closed entries
    kge_hparams hp;
    memset(&hp, 0, sizeof(hp));
    hp.model = KGE_PAIRRE; hp.d_e = 8; hp.d_r = 16;
    kge_hparams hd = hp;
    hd.model = KGE_DISTMULT; hd.d_r = 8;
    need = kge_step_workspace_bytes(&hp, 4, 1, 4, 3, 5, 2);
    EXPECT(need > kge_step_workspace_bytes(&hd, 4, 1, 4, 3, 5, 2));
    EXPECT(kge_step_workspace_bytes(&hp, 64, 2, 32, 40, 70, 3) > kge_step_workspace_bytes(&hd, 64, 2, 32, 40, 70, 3) + 2 * 64 * 8 * sizeof(float));
    kge_tables tb;
    memset(&tb, 0, sizeof(tb));
    kge_batch b;
    memset(&b, 0, sizeof(b));
    b.B = 4; b.C = 1; b.chunk = 4; b.N = 3; b.UE = 5; b.UR = 2;
    EXPECT(kge_step_fused(&hp, &tb, &b, nullptr, p, 1 << 20, nullptr) == KGE_ERR_ARG && !says("PairRE") && !says("unknown model"));
    kge_shards sh;
    memset(&sh, 0, sizeof(sh));
    EXPECT(kge_step_sharded(&hp, &sh, &b, nullptr, p, 1 << 20, nullptr) == KGE_ERR_ARG && says("PairRE") && says("kge_step_sharded"));
    kge_emit em;
    memset(&em, 0, sizeof(em));
    EXPECT(kge_step_grads(&hp, &tb, &b, nullptr, &em, p, 1 << 20, nullptr) == KGE_ERR_ARG && says("PairRE") && says("kge_step_grads"));
    kge_pipe *pipe = nullptr;
    EXPECT(kge_pipe_create(&pipe) == KGE_OK);
    EXPECT(kge_step_async(pipe, &hp, &tb, &b, nullptr, nullptr, p, 1 << 20, nullptr) == KGE_ERR_ARG && says("PairRE") && says("kge_step_async"));
    kge_pipe_destroy(pipe);
    kge_sampler_job job;
    memset(&job, 0, sizeof(job));
    EXPECT(kge_step_fused_sampling(&hp, &tb, &b, nullptr, p, 1 << 20, &job, nullptr) == KGE_ERR_ARG && says("PairRE") &&
           says("kge_step_fused_sampling"));
    EXPECT(kge_rank_eval_split(KGE_PAIRRE, 0, one, 5, one, 5, one, 2, nullptr, ids, ids, ids, 1, 8, 16, 0.f, 1.f, nullptr, 0, nullptr, nullptr, 1,
                               ranks, nullptr, p, 1 << 20, 0, nullptr) == KGE_ERR_ARG && says("PairRE") && says("kge_rank_eval_split"));
    EXPECT(kge_rank_rel_eval(KGE_PAIRRE, one, 5, one, 10, nullptr, ids, ids, ids, 4, 8, 16, 0.f, 1.f, ids, ids, 4, ranks, nullptr, p, 1 << 20, 0,
                             nullptr) == KGE_ERR_ARG && says("PairRE") && says("kge_rank_rel_eval"));
    EXPECT(kge_rank_rel_workspace_bytes(KGE_PAIRRE, 4, 10, 8, 16) == 0);
    printf("pairre_host_check: %d checks passed\n", n_checks);
    return 0;
}
