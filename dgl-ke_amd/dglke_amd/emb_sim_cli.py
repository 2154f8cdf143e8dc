"""dglke_emb_sim: top-K most similar embedding pairs - the reference's entry point (python/dglke/infer_emb_sim.py:27-70
flags, utils.py:162-200 id lists and mapping file, output layout :118-135), with EmbSimInfer (dglke_amd/infer.py) on the GPU."""
import argparse

from ._lib import KgeError
from .predict_cli import load_id_list, read_map

FORMATS = {'l_r': (True, True), 'l_*': (True, False), '*_r': (False, True), '*': (False, False)}
EXEC_MODES = {'pairwise': (True, False), 'all': (False, False), 'batch_left': (False, True)}     # -> (pair_ws, bcast)
SIM_FUNCS = ('cosine', 'l2', 'l1', 'dot', 'ext_jaccard')


class ArgParser(argparse.ArgumentParser):
    def __init__(self):
        super(ArgParser, self).__init__()
        a = self.add_argument
        a('--mfile', type=str, default=None)
        a('--emb_file', type=str, default=None)
        a('--format', type=str)
        a('--data_files', type=str, default=None, nargs='+')
        a('--raw_data', default=False, action='store_true')
        a('--exec_mode', type=str, default='all')
        a('--topK', type=int, default=10)
        a('--sim_func', type=str, default='cosine')
        a('--output', type=str, default='result.tsv')
        a('--gpu', type=int, default=-1)


def parse_inputs(args):
    """(left, right, id2e) from --format / --data_files / --raw_data (None = all)"""
    if args.format not in FORMATS:
        raise KgeError("unknown --format %r (one of %s)" % (args.format, ', '.join(FORMATS)))
    want = FORMATS[args.format]
    files = list(args.data_files or [])
    if len(files) != sum(want):
        raise KgeError("--format %s needs %d data files (got %d)" % (args.format, sum(want), len(files)))
    e2i = id2e = None
    if args.raw_data:
        if args.mfile is None:
            raise KgeError("When using RAW ID through --raw_data, mfile should be provided.")
        e2i, id2e = read_map(args.mfile)
    it = iter(files)
    left = load_id_list(next(it), e2i) if want[0] else None
    right = load_id_list(next(it), e2i) if want[1] else None
    return left, right, id2e


def write_tsv(path, result, id2e=None):
    with open(path, 'w+') as f:
        f.write('left\tright\tscore\n')
        for hl, tl, sl in result:
            for h, t, s in zip(hl.tolist(), tl.tolist(), sl.tolist()):
                if id2e is not None:
                    h, t = id2e[h], id2e[t]
                f.write('{}\t{}\t{}\n'.format(h, t, s))


def check_args(args):
    from .infer import check_k
    if args.gpu < 0:
        raise KgeError("dglke_emb_sim runs on the GPU only: pass --gpu <id> (there is no CPU path)")
    if args.exec_mode not in EXEC_MODES:
        raise KgeError("unknown --exec_mode %r (one of %s)" % (args.exec_mode, ', '.join(EXEC_MODES)))
    if args.sim_func not in SIM_FUNCS:
        raise KgeError("unknown --sim_func %r (one of %s)" % (args.sim_func, ', '.join(SIM_FUNCS)))
    check_k(args.topK)
    if args.emb_file is None:
        raise KgeError("--emb_file is required")
    left, right, id2e = parse_inputs(args)
    if args.exec_mode == 'pairwise' and not (left is not None and right is not None and len(left) == len(right)):
        raise KgeError("For pairwise execution mode, the left and right lists should have same length")
    return left, right, id2e


def main(argv=None):
    args = ArgParser().parse_args(argv)
    left, right, id2e = check_args(args)
    from .infer import EmbSimInfer
    import torch as th
    th.cuda.set_device(args.gpu)                   # (as dglke_eval: every call of this process goes to that GPU)
    pair_ws, bcast = EXEC_MODES[args.exec_mode]
    model = EmbSimInfer(args.gpu, args.emb_file, args.sim_func)
    model.load_emb()
    result = model.topK(left, right, bcast=bcast, pair_ws=pair_ws, k=args.topK)
    write_tsv(args.output, result, id2e)
    print('Inference Done')
    print('The result is saved in {}'.format(args.output))
