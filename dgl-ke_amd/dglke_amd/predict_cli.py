"""dglke_predict: top-K triples of a trained model - the reference's inference entry point (python/dglke/infer_score.py:27-77
flags, utils.py:60-160 id lists and mapping files, output layout :200-220), with ScoreInfer (dglke_amd/infer.py) on the GPU.
Reads the files dglke_train (this one or the reference's) writes: <model_path>/config.json and
<model_path>/<dataset>_<model>_{entity,relation}.npy."""
import argparse
import csv
import json
import os

from ._lib import KgeError

FORMATS = {          # format -> which of (head, rel, tail) come from --data_files, in order
    'h_r_t': (True, True, True), 'h_r_*': (True, True, False), 'h_*_t': (True, False, True), '*_r_t': (False, True, True),
    'h_*_*': (True, False, False), '*_r_*': (False, True, False), '*_*_t': (False, False, True)}
EXEC_MODES = ('triplet_wise', 'all', 'batch_head', 'batch_rel', 'batch_tail')


class ArgParser(argparse.ArgumentParser):
    def __init__(self):
        super(ArgParser, self).__init__()
        a = self.add_argument
        a('--model_path', type=str, default='ckpts')
        a('--format', type=str)
        a('--data_files', type=str, default=None, nargs='+')
        a('--raw_data', default=False, action='store_true')
        a('--exec_mode', type=str, default='all')
        a('--topK', type=int, default=10)
        a('--score_func', type=str, default='none')
        a('--output', type=str, default='result.tsv')
        a('--entity_mfile', type=str, default=None)
        a('--rel_mfile', type=str, default=None)
        a('--gpu', type=int, default=-1)


def read_lines(path):
    """one id (or raw name) per line, as utils.py reads them (the line without its newline)"""
    out = []
    with open(path, 'r') as f:
        for line in f:
            out.append(line[:-1] if line.endswith('\n') else line)
    return out


def read_map(path):
    """an id mapping file (id<TAB>name per row): name -> id, id -> name"""
    n2i, i2n = {}, {}
    with open(path, 'r') as f:
        for row in csv.reader(f, delimiter='\t'):
            n2i[row[1]] = int(row[0])
            i2n[int(row[0])] = row[1]
    return n2i, i2n


def load_id_list(path, name2id=None):
    import numpy as np
    vals = read_lines(path)
    if name2id is None:
        return np.asarray([int(v) for v in vals], dtype=np.int64)
    try:
        return np.asarray([name2id[v] for v in vals], dtype=np.int64)
    except KeyError as e:
        raise KgeError("%s: %s is not in the mapping file" % (path, e))


def load_model_config(path):
    """utils.py:30-49: the keys ScoreInfer needs from <model_path>/config.json"""
    if not os.path.exists(path):
        raise KgeError("no model config: %s" % path)
    with open(path, 'r') as f:
        c = json.load(f)
    return {k: c[k] for k in ('model_name', 'dataset', 'hidden_dim', 'gamma', 'double_ent', 'double_rel')}


def parse_inputs(args):
    """(head, rel, tail, id2e, id2r) from --format / --data_files / --raw_data (None = all)"""
    if args.format not in FORMATS:
        raise KgeError("unknown --format %r (one of %s)" % (args.format, ', '.join(FORMATS)))
    want = FORMATS[args.format]
    files = list(args.data_files or [])
    if len(files) != sum(want):
        raise KgeError("--format %s needs %d data files (got %d)" % (args.format, sum(want), len(files)))
    e2i = r2i = id2e = id2r = None
    if args.raw_data:
        if args.entity_mfile is None or args.rel_mfile is None:
            raise KgeError("When using RAW ID through --raw_data, entity_mfile and rel_mfile should be provided.")
        e2i, id2e = read_map(args.entity_mfile)
        r2i, id2r = read_map(args.rel_mfile)
    it = iter(files)
    head = load_id_list(next(it), e2i) if want[0] else None
    rel = load_id_list(next(it), r2i) if want[1] else None
    tail = load_id_list(next(it), e2i) if want[2] else None
    return head, rel, tail, id2e, id2r


def write_tsv(path, result, id2e=None, id2r=None):
    """infer_score.py:200-220: header, then one line per result; names under --raw_data; scores through .tolist()"""
    with open(path, 'w+') as f:
        f.write('head\trel\ttail\tscore\n')
        for hl, rl, tl, sl in result:
            for h, r, t, s in zip(hl.tolist(), rl.tolist(), tl.tolist(), sl.tolist()):
                if id2e is not None:
                    h, r, t = id2e[h], id2r[r], id2e[t]
                f.write('{}\t{}\t{}\t{}\n'.format(h, r, t, s))


def check_args(args):
    """every refusal that needs no device, before the device is touched"""
    from .infer import check_k
    if args.gpu < 0:
        raise KgeError("dglke_predict runs on the GPU only: pass --gpu <id> (there is no CPU path)")
    if args.exec_mode not in EXEC_MODES:
        raise KgeError("unknown --exec_mode %r (one of %s)" % (args.exec_mode, ', '.join(EXEC_MODES)))
    if args.score_func not in ('none', 'logsigmoid'):
        raise KgeError("unknown --score_func %r (none or logsigmoid)" % (args.score_func,))
    check_k(args.topK)
    config = load_model_config(os.path.join(args.model_path, 'config.json'))
    if config['model_name'] == 'TransR':
        raise KgeError("TransR has no inference path (the reference's InferModel refuses it too)")
    from .train import check_model_widths
    check_model_widths(config['model_name'], config['hidden_dim'], config['double_ent'], config['double_rel'])
    head, rel, tail, id2e, id2r = parse_inputs(args)
    if args.exec_mode == 'triplet_wise' and not (head is not None and rel is not None and tail is not None and
                                                 len(head) == len(rel) == len(tail)):
        raise KgeError("For triplet wise execution mode, head, relation and tail lists should have same length")
    return config, head, rel, tail, id2e, id2r


def main(argv=None):
    args = ArgParser().parse_args(argv)
    config, head, rel, tail, id2e, id2r = check_args(args)
    from .infer import ScoreInfer
    import torch as th
    th.cuda.set_device(args.gpu)                   # (as dglke_eval: every call of this process goes to that GPU)
    model = ScoreInfer(args.gpu, config, args.model_path, args.score_func)
    model.load_model()
    result = model.topK(head, rel, tail, args.exec_mode, args.topK)
    write_tsv(args.output, result, id2e, id2r)
    print('Inference Done')
    print('The result is saved in {}'.format(args.output))
