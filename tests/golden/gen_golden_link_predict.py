#!/usr/bin/env python3
"""Golden vectors for link prediction with known-edge exclusion: runs the UNMODIFIED reference `link_predict`
(python/dglke/models/ke_model.py:205-641) on CPU through the same dgl stubs as gen_golden.py / gen_golden_infer.py.

TEST INFRASTRUCTURE ONLY; runs in the build container only (needs the reference).  The reference asks a DGLGraph for the
edges between node pairs; the stand-in below subclasses the stub's `dgl._deprecate.graph.DGLGraph` (link_predict asserts the
type) and answers `edge_ids(u, v, return_uv=True)` and `edata['tid']` from the known triples.

link_predict/lp_<model>.npz: small seeded tables saved as the reference loads them (entity.npy / relation.npy), the known
triples - the 2K best combinations of every head by the reference's own scores plus random ones, so that 'exclude' has work
to do - and for sfunc in {none, logsigmoid}, every broadcast exec mode and exclude_mode in {None, mask, exclude}: the
reference's result tuples (concatenated; `<key>_n` = the length of each group's tuple; `_m` = the mask) and its full score
vector [H*R*T]."""
import os
import sys
import tempfile

import numpy as np
import torch as th

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_predict")
MODES = ("all", "batch_head", "batch_rel", "batch_tail")
MODELS = {"TransE_l2": (12, 5, 71), "DistMult": (32, 5, 72)}          # model: (hidden, K, seed)


def make_graph(kh, kr, kt):
    import dgl

    class Graph(dgl._deprecate.graph.DGLGraph):
        def __init__(self):
            self.edata = {"tid": th.tensor(kr)}
            self._by_pair = {}
            for e, (a, b) in enumerate(zip(kh.tolist(), kt.tolist())):
                self._by_pair.setdefault((a, b), []).append(e)

        def edge_ids(self, u, v, return_uv=False):
            uid, vid, eid = [], [], []
            for a, b in zip(th.as_tensor(u).reshape(-1).tolist(), th.as_tensor(v).reshape(-1).tolist()):
                for e in self._by_pair.get((a, b), ()):
                    uid.append(a); vid.append(b); eid.append(e)
            out = tuple(th.tensor(x, dtype=th.int64) for x in (uid, vid, eid))
            return out if return_uv else out[2]
    return Graph()


def _flat(res):
    out = {"n": np.array([len(tup[3]) for tup in res], np.int64)}
    for c, name in enumerate(("h", "r", "t", "s")):
        out[name] = np.concatenate([np.asarray(tup[c]).reshape(-1)[:len(tup[3])] for tup in res])
    if res and res[0][4] is not None:
        out["m"] = np.concatenate([np.asarray(tup[4]).reshape(-1) for tup in res])
    return out


def run_model(model, spec):
    from dglke.models import ke_model as KM
    hidden, K, seed = spec
    rng = np.random.RandomState(seed)
    n_ent, n_rel, gamma = 64, 6, 8.0
    ent = rng.uniform(-1, 1, (n_ent, hidden)).astype(np.float32)
    rel = rng.uniform(-1, 1, (n_rel, hidden)).astype(np.float32)
    tmp = tempfile.mkdtemp()
    np.save(os.path.join(tmp, "entity.npy"), ent)
    np.save(os.path.join(tmp, "relation.npy"), rel)
    cls = getattr(KM, model + "Model")
    m = cls(th.device("cpu"), gamma) if model.startswith("TransE") else cls(th.device("cpu"))
    m.load(tmp)
    h = rng.choice(n_ent, 6, replace=False)
    r = rng.choice(n_rel, 3, replace=False)
    t = rng.choice(n_ent, 40, replace=False)
    with th.no_grad():
        raw = m._infer_score_func(th.tensor(h), th.tensor(r), th.tensor(t))
    out = {"entity": ent, "relation": rel, "gamma": np.float64(gamma), "K": np.int64(K), "h": h, "r": r, "t": t,
           "none_full": raw.numpy().astype(np.float32).reshape(-1),
           "logsigmoid_full": th.nn.functional.logsigmoid(raw).numpy().astype(np.float32).reshape(-1)}
    S = raw.numpy().reshape(len(h), -1)
    kh, kr, kt = [], [], []
    for i in range(len(h)):
        best = np.argsort(-S[i], kind="stable")[:2 * K]
        kh += [h[i]] * len(best); kr += list(r[best // len(t)]); kt += list(t[best % len(t)])
    kh += list(rng.randint(0, n_ent, 600)); kr += list(rng.randint(0, n_rel, 600)); kt += list(rng.randint(0, n_ent, 600))
    kh, kr, kt = (np.array(x, np.int64) for x in (kh, kr, kt))
    out.update(known_h=kh, known_r=kr, known_t=kt)
    m.attach_graph(make_graph(kh, kr, kt))
    for sfunc in ("none", "logsigmoid"):
        for mode in MODES:
            for emode in (None, "mask", "exclude"):
                res = m.link_predict(h, r, t, exec_mode=mode, sfunc=sfunc, topk=K, exclude_mode=emode)
                for key, v in _flat(res).items():
                    out["%s_%s_%s_%s" % (sfunc, mode, emode, key)] = v
    path = os.path.join(OUT, "lp_%s.npz" % model.lower())
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def main():
    G.install_stubs()
    import dgl.backend as F
    F.unsqueeze = lambda t, dim: th.unsqueeze(t, dim)
    sys.path.insert(0, G.REF)
    th.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    only = sys.argv[1:]
    for model, spec in MODELS.items():
        if not only or model in only:
            run_model(model, spec)


if __name__ == "__main__":
    main()
