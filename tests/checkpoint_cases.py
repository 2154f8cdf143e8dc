"""Case table of tests/test_gpu_checkpoint.py (checked on the CPU by tests/test_checkpoint_inputs.py): the restarts that must
reproduce an uninterrupted run bit for bit.  Shape, planted graph and command line are those of tests/train_loop_cases.py (230
steps of batch 64 x 16 negatives at hidden 32 over 4000 training triples: epochs open at steps 63, 125 and 187).

Protocol of a case: run A trains `--max_step 230` without either flag; run B1 trains `--max_step K --checkpoint_interval K`; run
B2 is `--resume <B1's run directory> --max_step 230`.  A chained case has several K: every run but the first resumes its
predecessor, every run but the last checkpoints at its own K."""
import train_loop_cases as L

MAX_STEP, EPOCH = L.MAX_STEP, L.EPOCH
LOOP = (20, 50)             # --graph_steps, --log_interval of the cases that do not say otherwise

# (id, model, flags of every run, weighted data directory, [K...], --graph_steps of B1 / of the resumed runs)
CASES = [
    ("odd_step", "TransE_l2", [], False, [45], (20, 20)),             # odd, no multiple of the group, no log mark
    ("epoch_opens", "TransE_l2", [], False, [124], (20, 20)),         # even; step 125 is the first batch of an epoch
    ("graphs_to_eager", "TransE_l2", [], False, [100], (20, 0)),
    ("adam", "TransE_l2", ["--optimizer", "Adam", "--lr", "0.001"], False, [45], (20, 20)),
    ("transr", "TransR", ["--lr", "0.05"], False, [45], (20, 20)),
    ("host_sampler", "TransE_l2", ["--has_edge_importance"], True, [100], (20, 20)),   # 38 batches into its second permutation
    ("subsampling", "TransE_l2", ["--subsampling_weight"], False, [45], (20, 20)),
    ("exclude_positive", "TransE_l2", ["--exclude_positive"], False, [45], (20, 20)),
    ("chained", "TransE_l2", [], False, [45, 124], (20, 20)),         # the middle run is itself resumed, and checkpoints
]
CASE_IDS = [c[0] for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def n_tables(c):
    """tables that must come back bit for bit: rows and state of both sides, TransR's projection and its state, Adam's moments"""
    return 4 + (2 if c[1] == "TransR" else 0) + (2 if "Adam" in c[2] else 0)


def argv_a(c, data, save):
    """run A"""
    return L.argv(data, save, c[1], c[5][0], LOOP[1], c[2])


def argv_b(c, data, save, i, resume=None, extra=()):
    """run i of the chain B: i = 0 checkpoints at K[0]; 0 < i < len(K) resumes its predecessor and checkpoints at K[i]; i = len(K)
    resumes the last checkpoint and trains to max_step.  resume: the predecessor's run directory"""
    ks = c[4]
    last = i == len(ks)
    a = L.argv(data, save, c[1], c[5][0] if i == 0 else c[5][1], LOOP[1], list(c[2]) + list(extra), MAX_STEP if last else ks[i])
    if not last:
        a += ["--checkpoint_interval", str(ks[i])]
    if i > 0:
        a += ["--resume", resume]
    return a
