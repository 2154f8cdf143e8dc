"""Mid-run checkpoints of `dglke_train` (`--checkpoint_interval N`) and the restart from one (`--resume PATH`).

A checkpoint is a directory that is also a model directory: config.json and the tables under the names `save_emb` uses (so
`dglke_eval`, `dglke_predict` and `ke_model.*.load` read `RUN/checkpoint` like any saved model), plus what a restart needs to
continue the SAME sequence of steps bit for bit: the optimizer's state tables (Adagrad's running mean squares / Adam's per-row counts
and moment tables, TransR's projection state), every lane's sampler state and loss sums, the step and the steps since the last log
line.  What is a function of `--seed` and the dataset - the device sampler's base permutation, subsampling weights, the
known-triple index, the lanes' partition - is rebuilt, not stored.

Layers, bottom up:
  file layer      .npy files written and read in row blocks (byte for byte np.save's files, bounded host staging), the
                  write-to-`checkpoint.tmp`-then-rename protocol, `checkpoint.json` with per-file shape / dtype / size, `find_latest`;
                  works on CPU tensors and arrays, nothing here touches a GPU at import;
  compatibility   which flags of the saved and the given run must agree (`check_compatible`), a pure function of two namespaces;
  trainer layer   `save_trainer` / `restore_trainer` of a one-GPU `train.Trainer`.
"""
import json
import os
import re
import shutil
import time

import numpy as np

from ._lib import KgeError

FORMAT_VERSION = 1
META = 'checkpoint.json'
CURRENT, PREVIOUS, PARTIAL = 'checkpoint', 'checkpoint.old', 'checkpoint.tmp'
# host staging of one copy between a table and its file, whatever the table's size
BLOCK_BYTES = 64 << 20

# flags that decide the sequence of batches or the layout of what is stored: a restart must repeat them
MUST_EQUAL = ('model_name', 'hidden_dim', 'double_ent', 'double_rel', 'optimizer',
              'num_proc', 'batch_size', 'neg_sample_size', 'seed',
              'has_edge_importance', 'subsampling_weight', 'edge_importance_on_device',
              'dataset')
# flags that say where a run reads and writes, not what it computes: never reported as a difference
_BOOKKEEPING = ('save_path', 'resume')


class FutureFormat(KgeError):
    """a checkpoint.json written by a later build"""


# ---- file layer ------------------------------------------------------------------------------------------------------------

def _is_tensor(x):
    return hasattr(x, 'numpy') and hasattr(x, 'element_size')


def _np_dtype(src):
    if _is_tensor(src):
        import torch
        return torch.empty(0, dtype=src.dtype).numpy().dtype
    return np.asarray(src).dtype


def write_npy_blocks(path, src, block_bytes=BLOCK_BYTES):
    """write the tensor (any device) or array `src` as the .npy file np.save would write, row block by row block: the file is
    created at its full shape (np.lib.format.open_memmap) and filled through ONE host staging buffer of at most block_bytes
    (at least one row), reused block after block - no second device copy of a table, no host copy of a whole table.  Returns
    the file's size in bytes."""
    if not _is_tensor(src):
        src = np.asarray(src)
    shape = tuple(int(x) for x in src.shape)
    dtype = _np_dtype(src)
    mm = np.lib.format.open_memmap(path, mode='w+', dtype=dtype, shape=shape)
    n = shape[0] if shape else 0
    if not shape:
        mm[...] = src.cpu().numpy() if _is_tensor(src) else np.asarray(src)
    elif mm.size:
        row_bytes = (mm.size // n) * dtype.itemsize
        per = max(1, min(n, int(block_bytes) // row_bytes))
        if _is_tensor(src):
            import torch
            buf = torch.empty((per,) + shape[1:], dtype=src.dtype)
            for a in range(0, n, per):
                b = min(n, a + per)
                buf[:b - a].copy_(src[a:b])
                mm[a:b] = buf[:b - a].numpy()
        else:
            for a in range(0, n, per):
                mm[a:a + per] = src[a:a + per]
    mm.flush()
    del mm
    return os.path.getsize(path)


def read_npy_blocks(path, dst, block_bytes=BLOCK_BYTES):
    """fill the tensor `dst` (any device) IN PLACE from the .npy file, read through a memory map in row blocks of at most
    block_bytes; shape and dtype must be the tensor's"""
    import torch
    mm = np.load(path, mmap_mode='r')
    if tuple(mm.shape) != tuple(dst.shape) or mm.dtype != _np_dtype(dst):
        raise KgeError("%s holds %s %s, expected %s %s" % (path, mm.dtype, tuple(mm.shape), _np_dtype(dst), tuple(dst.shape)))
    n = int(dst.shape[0]) if dst.dim() else 0
    if n and mm.size:
        per = max(1, int(block_bytes) // ((mm.size // n) * mm.dtype.itemsize))
        for a in range(0, n, per):
            dst[a:a + per].copy_(torch.from_numpy(np.array(mm[a:a + per])))      # (one block in host memory)
    del mm


def npy_header(path):
    """(shape, dtype string) of a .npy file from its header alone"""
    with open(path, 'rb') as f:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        shape, fortran, dtype = read(f)
    if fortran:
        raise ValueError("Fortran order")
    return tuple(int(x) for x in shape), np.dtype(dtype).str


def file_entry(path):
    """what checkpoint.json records of a .npy file"""
    shape, dtype = npy_header(path)
    return dict(shape=list(shape), dtype=dtype, bytes=os.path.getsize(path))


def read_meta(ckpt_dir):
    """checkpoint.json of a checkpoint directory.  Raises KgeError if there is none that can be read (an interrupted write leaves
    none: the file is written last), or if it is of a format this build does not know."""
    f = os.path.join(ckpt_dir, META)
    try:
        with open(f) as fh:
            meta = json.load(fh)
        version, step = int(meta['format_version']), int(meta['step'])
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise KgeError("no readable %s in %s (%s)" % (META, ckpt_dir, e))
    if version > FORMAT_VERSION:
        raise FutureFormat("%s is of checkpoint format %d, this build reads formats up to %d" % (f, version, FORMAT_VERSION))
    if step < 0:
        raise KgeError("%s: step %d" % (f, step))
    return meta


def verify_files(ckpt_dir, meta):
    """every file checkpoint.json lists is there with the recorded size, shape and dtype; the first that is not is refused by
    name (contents are not checksummed)"""
    for name, want in sorted(meta['files'].items()):
        f = os.path.join(ckpt_dir, name)
        if not os.path.isfile(f):
            raise KgeError("checkpoint file %s is missing" % f)
        size = os.path.getsize(f)
        if size != int(want['bytes']):
            raise KgeError("checkpoint file %s has %d bytes, %s records %d" % (f, size, META, int(want['bytes'])))
        try:
            shape, dtype = npy_header(f)
        except Exception as e:       # noqa: BLE001 - whatever the header parser raises on a damaged file
            raise KgeError("checkpoint file %s has no readable .npy header (%s)" % (f, e))
        if list(shape) != [int(x) for x in want['shape']] or dtype != want['dtype']:
            raise KgeError("checkpoint file %s holds %s %s, %s records %s %s"
                           % (f, dtype, list(shape), META, want['dtype'], list(want['shape'])))


def locate(path, log=print):
    """the checkpoint `--resume PATH` names: PATH itself if it holds checkpoint.json, else PATH/checkpoint, else - a write was
    interrupted between its two renames, or the newest one is unreadable - PATH/checkpoint.old, which is said.  Returns
    (checkpoint directory, its checkpoint.json); refuses if there is none.  A checkpoint of a newer format is refused, not
    skipped."""
    if not os.path.isdir(path):
        raise KgeError("--resume: %s is not a directory" % path)
    if os.path.isfile(os.path.join(path, META)):
        return path, read_meta(path)
    cur, old = os.path.join(path, CURRENT), os.path.join(path, PREVIOUS)
    if os.path.isfile(os.path.join(cur, META)):
        try:
            return cur, read_meta(cur)
        except FutureFormat:
            raise
        except KgeError as e:
            why = str(e)
    else:
        why = "no %s in %s" % (META, cur)
    if os.path.isfile(os.path.join(old, META)):
        meta = read_meta(old)
        log("--resume: %s; using the previous checkpoint %s (step %d)" % (why, old, int(meta['step'])))
        return old, meta
    raise KgeError("--resume: %s holds no readable checkpoint (%s, and no %s)" % (path, why, os.path.join(PREVIOUS, META)))


def find_latest(save_path, model_name, dataset):
    """the run directory `--resume latest` takes: of the `<model>_<dataset>_<n>` folders under save_path the one with the highest
    n that holds a readable checkpoint (folders without one - a run that never reached a mark - are skipped); None if there is
    none, or no save_path"""
    if not os.path.isdir(save_path):
        return None
    pat = re.compile(re.escape('{}_{}_'.format(model_name, dataset)) + r'(\d+)$')
    runs = sorted(((int(m.group(1)), m.group(0)) for m in map(pat.match, os.listdir(save_path)) if m), reverse=True)
    for _, name in runs:
        run = os.path.join(save_path, name)
        try:
            locate(run, log=lambda _m: None)
        except KgeError:
            continue
        return run
    return None


def write_checkpoint(run_dir, tensors, meta, config=None, block_bytes=BLOCK_BYTES):
    """write one checkpoint of `run_dir`: the files `tensors` (file name -> tensor or array) in row blocks, config.json (`config`:
    a callable that writes it into the directory it is given), and checkpoint.json = `meta` + the format version + the per-file
    records, LAST, all into `checkpoint.tmp/`; then the standing `checkpoint/` becomes `checkpoint.old/`, the new one takes its
    place and the old one is removed - at every instant one of the two holds a complete checkpoint, which is what `locate`
    looks for.  Only the newest is kept.  Returns the bytes written."""
    tmp, cur, old = (os.path.join(run_dir, n) for n in (PARTIAL, CURRENT, PREVIOUS))
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)
    os.makedirs(tmp)
    files, total = {}, 0
    for name, t in tensors.items():
        total += write_npy_blocks(os.path.join(tmp, name), t, block_bytes)
        files[name] = file_entry(os.path.join(tmp, name))
    if config is not None:
        config(tmp)
        total += os.path.getsize(os.path.join(tmp, 'config.json'))
    doc = dict(meta)
    doc['format_version'] = FORMAT_VERSION
    doc['files'] = files
    part = os.path.join(tmp, META + '.part')
    with open(part, 'w') as f:
        json.dump(doc, f)
        f.flush()
        os.fsync(f.fileno())
    os.rename(part, os.path.join(tmp, META))
    total += os.path.getsize(os.path.join(tmp, META))
    if os.path.isdir(cur):
        if os.path.isdir(old):                  # left by a write that was interrupted after its second rename
            shutil.rmtree(old)
        os.rename(cur, old)
    os.rename(tmp, cur)
    if os.path.isdir(old):
        shutil.rmtree(old)
    return total


# ---- flags -----------------------------------------------------------------------------------------------------------------

def check_flags(args):
    """--checkpoint_interval and --resume store and restore the state of ONE GPU's strict step: refuse, before anything is
    loaded or created, what has other state"""
    n, resume = getattr(args, 'checkpoint_interval', 0) or 0, getattr(args, 'resume', None)
    if n < 0:
        raise KgeError("--checkpoint_interval must not be negative (got %d; 0 writes none)" % n)
    if not n and not resume:
        return
    flag = "--checkpoint_interval" if n else "--resume"
    if len(args.gpu) > 1:
        raise KgeError("%s is not available on more than one GPU (--gpu takes one entry): the sharded trainers' tables are not "
                       "checkpointed" % flag)
    if args.async_update_pipeline:
        raise KgeError("%s is not available with --async_update_pipeline (a one-step-stale pipeline carries a pending update "
                       "between steps); plain --async_update runs the strict step and is fine" % flag)
    if args.async_update_rel:
        raise KgeError("%s is not available with --async_update_rel (a one-step-stale pipeline carries a pending update between "
                       "steps); plain --async_update runs the strict step and is fine" % flag)


def check_max_step(max_step, step):
    if max_step <= step:
        raise KgeError("--resume: the checkpoint is at step %d and --max_step is %d: nothing is left to train (pass a --max_step "
                       "above %d)" % (step, max_step, step))


def check_compatible(saved, given, saved_parsed=None):
    """a restart continues the saved run's sequence of batches on the saved run's tables: the flags of MUST_EQUAL agree (saved:
    the namespace in checkpoint.json, given: this command line's; --batch_size of both after get_compatible_batch_size) or the
    first that does not is refused with both values.  Every other flag may differ and the command line wins; returns those that
    do as [(key, saved value, given value)], compared against the saved run's command line as it was parsed (saved_parsed;
    default: saved) so that values the run derived later - an evaluation's candidate count - do not show up as changes."""
    from .train import get_compatible_batch_size
    saved, given = dict(saved), dict(given)

    def norm(ns):
        ns = dict(ns)
        if ns.get('batch_size') is not None and ns.get('neg_sample_size'):
            ns['batch_size'] = get_compatible_batch_size(ns['batch_size'], ns['neg_sample_size'], quiet=True)
        return ns
    s, g = norm(saved), norm(given)
    for key in MUST_EQUAL:
        if key not in s:
            raise KgeError("--resume: the checkpoint does not record --%s" % key)
        if s[key] != g.get(key):
            raise KgeError("--resume: --%s is %r in the checkpoint and %r on this command line; a restart must repeat it"
                           % (key, s[key], g.get(key)))
    parsed = dict(saved if saved_parsed is None else saved_parsed)
    changed = []
    for key in sorted(given):
        if key in MUST_EQUAL or key in _BOOKKEEPING:
            continue
        if key in parsed and parsed[key] != given[key]:
            changed.append((key, parsed[key], given[key]))
    return changed


class Resume(object):
    """a checkpoint opened for a restart: its directory, its checkpoint.json, the step it stands at"""

    def __init__(self, path, meta):
        self.path, self.meta = path, meta
        self.step, self.since_log = int(meta['step']), int(meta['since_log'])


def open_resume(args, log=print):
    """`--resume` as far as it goes without the dataset or a GPU: find the checkpoint ('latest': the newest run under
    --save_path, None - a fresh run - if there is none), check its files against checkpoint.json, the flags against its
    namespace and --max_step against its step.  Reads only."""
    path = args.resume
    if path == 'latest':
        path = find_latest(args.save_path, args.model_name, args.dataset)
        if path is None:
            log("--resume latest: no checkpoint of {}_{}_<n> under {}: starting a fresh run".format(
                args.model_name, args.dataset, args.save_path))
            return None
    ckpt_dir, meta = locate(path, log)
    verify_files(ckpt_dir, meta)
    changed = check_compatible(meta['args'], vars(args), meta.get('args_parsed'))
    check_max_step(args.max_step, int(meta['step']))
    log("--resume: {} at step {} of the run's {}".format(ckpt_dir, int(meta['step']), meta['args'].get('max_step')))
    for key, was, now in changed:
        log("--resume: --{} was {!r} in the checkpointed run, is {!r} now".format(key, was, now))
    return Resume(ckpt_dir, meta)


# ---- a one-GPU Trainer -----------------------------------------------------------------------------------------------------

def table_files(trainer):
    """file name -> live tensor of everything the trainer's engines train: the model tables under save_emb's names, the state
    tables and Adam's moment tables beside them"""
    args = trainer.args
    stem = '{}_{}'.format(args.dataset, args.model_name)
    suffix = {'entity': '_entity', 'relation': '_relation', 'projection': 'projection',
              'entity_state': '_entity_state', 'relation_state': '_relation_state', 'projection_state': 'projection_state',
              'entity_mom': '_entity_mom', 'relation_mom': '_relation_mom'}
    return {name: (stem + suffix[name] + '.npy', t) for name, t in trainer.model.engine.named_tensors().items()}


def _lane_files(k):
    return 'lane%d_loss_accum.npy' % k, 'lane%d_sampler_perm.npy' % k


def save_trainer(trainer, step, since_log, parsed=None):
    """one checkpoint of a one-GPU trainer into <run directory>/checkpoint, between two steps: the caller has synchronised.
    Returns (bytes, seconds)."""
    import torch
    from . import _lib
    from .train import write_config
    t0 = time.time()
    args, ds = trainer.args, trainer.dataset
    torch.cuda.synchronize()
    tensors = {fname: t for fname, t in table_files(trainer).values()}
    lanes = []
    for lane in trainer.lanes:
        acc_file, perm_file = _lane_files(lane.k)
        st = lane.sampler.get_state()
        if st['kind'] == 'host':                # the current permutation is an array of the split's size: a file, not JSON
            perm = st.pop('perm')
            st['perm_file'] = None
            if perm is not None:
                st['perm_file'] = perm_file
                tensors[perm_file] = perm
        tensors[acc_file] = lane.engine.loss_accum
        lanes.append(dict(lane=lane.k, sampler=st, loss_accum_file=acc_file))
    meta = dict(step=int(step), since_log=int(since_log), args=dict(vars(args)),
                args_parsed=dict(parsed) if parsed is not None else dict(vars(args)),
                n_entities=int(ds.n_entities), n_relations=int(ds.n_relations), n_train=int(len(ds.train[0])),
                abi_version=int(_lib.KGE_ABI_VERSION), torch_version=str(torch.__version__), lanes=lanes)
    total = write_checkpoint(args.save_path, tensors, meta,
                             config=lambda d: write_config(args, ds.emap_fname, ds.rmap_fname, path=d))
    return total, time.time() - t0


def restore_trainer(trainer, resume):
    """put every piece of state of the checkpoint back into a freshly built trainer, in place: tables, states and moments (read
    from the memory-mapped files in row blocks into the tensors the engines, lanes and later graphs hold), every lane's sampler
    state and loss sums.  The dataset must be the checkpointed run's."""
    import torch
    from . import _lib
    meta, d, ds = resume.meta, resume.path, trainer.dataset
    for key, have in (('n_entities', ds.n_entities), ('n_relations', ds.n_relations), ('n_train', len(ds.train[0]))):
        if int(meta[key]) != int(have):
            raise KgeError("--resume: the checkpointed run had %s = %d, this dataset has %d" % (key, int(meta[key]), int(have)))
    if int(meta.get('abi_version', _lib.KGE_ABI_VERSION)) != _lib.KGE_ABI_VERSION:
        raise KgeError("--resume: the checkpoint was written by a library of ABI %s, this one is ABI %d"
                       % (meta.get('abi_version'), _lib.KGE_ABI_VERSION))
    if len(meta['lanes']) != len(trainer.lanes):
        raise KgeError("--resume: the checkpoint holds %d lanes, the trainer has %d" % (len(meta['lanes']), len(trainer.lanes)))
    files = table_files(trainer)
    for name, (fname, _) in files.items():
        if fname not in meta['files']:
            raise KgeError("--resume: the checkpoint has no %s (%s)" % (fname, name))
    maps = {name: np.load(os.path.join(d, fname), mmap_mode='r') for name, (fname, _) in files.items()}
    trainer.model.engine.load_named(maps, block_bytes=BLOCK_BYTES)
    del maps
    for lane, rec in zip(trainer.lanes, meta['lanes']):
        st = dict(rec['sampler'])
        want = 'device' if trainer.device_sampler else 'host'
        if st.get('kind') != want:
            raise KgeError("--resume: lane %d was fed by the %s sampler, this run's is the %s sampler" % (lane.k, st.get('kind'), want))
        if st['kind'] == 'host':
            st['perm'] = None if st.get('perm_file') is None else np.load(os.path.join(d, st['perm_file']))
        lane.sampler.set_state(st)
        read_npy_blocks(os.path.join(d, rec['loss_accum_file']), lane.engine.loss_accum)
    torch.cuda.synchronize()
    if str(meta.get('torch_version')) != str(torch.__version__):
        print("--resume: the checkpoint was written under torch {}, this is {}: the restart is bit-exact on the same build "
              "only".format(meta.get('torch_version'), torch.__version__))
