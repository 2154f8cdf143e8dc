"""The stream contract of include/kge_hip.h ("no allocation, no host synchronisation and no global mutable state inside; every call
takes an explicit stream ... and only enqueues kernels on it, so calls can be captured into a hipGraph"), as a table and helpers.
Their CPU checks: tests/test_stream_inputs.py; the GPU runs: tests/test_gpu_stream_contract.py.

STREAM_ENTRIES names every exported function whose prototype has a `void *` parameter named `stream` or ending in `_stream`
(`void *hip_stream`) and the GPU case(s) - test functions of
test_gpu_stream_contract.py without their `test_` - that run it on torch's default stream, on a side stream, and captured alone into
a graph that is replayed on the side stream (kge_step_phase and kge_step_async also run in test_two_engines_two_streams, which is
no three-mode case).  The helpers below read the C sources the way the CPU checks need them: comments and
string literals blanked, `#ifdef KGE_TIMELINE` blocks (the developer timeline, compiled out of the product) cut out, calls split
into their arguments by matching parentheses.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kge_hip.h")
CSRC = os.path.join(ROOT, "dgl-ke_amd", "csrc")


class Exempt(object):
    """an entry that is not run in the three modes, and the one-line reason"""

    def __init__(self, reason):
        self.reason = reason


MAX_EXEMPT = 3

STREAM_ENTRIES = {
    # the training steps
    "kge_step_fused": ["step_fused"],
    "kge_step_phase": ["step_phase"],
    "kge_step_async": ["step_async_group"],
    "kge_step_async_flush": ["step_async_group"],
    "kge_step_sharded": ["step_sharded"],
    "kge_step_fused_known": ["step_fused_known"],
    "kge_step_phase_known": ["step_phase_known"],
    "kge_known_neg_mask": ["known_neg_mask"],
    "kge_step_fused_sampling": ["step_fused_sampling"],
    "kge_sample_batches": ["step_fused_sampling"],
    "kge_step_grads": ["step_grads"],
    "kge_step_optim": ["step_optim_adam", "step_optim_adagrad"],
    "kge_sample_batches_weighted": ["sample_batches_weighted"],
    "kge_subsampling_weights": ["subsampling_weights"],
    "kge_reduce_loss": ["reduce_loss"],
    # the per-op entries behind dglke_amd.ops
    "kge_gather_rows": ["gather_and_scatter_rows"],
    "kge_scatter_add_rows": ["gather_and_scatter_rows"],
    "kge_score_pos": ["score_pos"],
    "kge_score_pos_bwd": ["score_pos"],
    "kge_score_neg_fwd": ["score_neg"],
    "kge_score_neg_bwd": ["score_neg"],
    "kge_loss_fwd_bwd": ["loss_fwd_bwd"],
    "kge_adagrad_scatter": ["adagrad_scatter"],
    "kge_pnorm_pow": ["pnorm_pow"],
    "kge_pnorm_pow_bwd": ["pnorm_pow"],
    "kge_mask_diag": ["mask_diag"],
    "kge_rank_from_scores": ["rank_from_scores"],
    "kge_transr_project": ["transr_projections"],
    "kge_transr_project_bwd": ["transr_projections"],
    "kge_transr_project_neg": ["transr_projections"],
    "kge_transr_project_neg_bwd": ["transr_projections"],
    # ranking
    "kge_rank_eval": ["rank_eval_split_and_plain"],
    "kge_rank_eval_split": ["rank_eval_split_and_plain"],
    "kge_rank_eval_ex": ["rank_eval_ex"],
    "kge_rank_eval_chunked": ["rank_eval_chunked"],
    "kge_rank_rel_eval": ["rank_rel_eval"],
    # top-K and inference
    "kge_topk_select": ["topk_select"],
    "kge_topk_select_filtered": ["topk_select"],
    "kge_topk_vector": ["topk_vector"],
    "kge_sim_pairwise": ["sim_pairwise"],
    "kge_triples_known": ["triples_known"],
    # the owner side and the routing of the range-sharded step
    "kge_adagrad_apply_rows": ["adagrad_apply_rows_and_packed"],
    "kge_adagrad_apply_packed": ["adagrad_apply_rows_and_packed"],
    "kge_adagrad_apply_merged": ["adagrad_apply_merged"],
    "kge_adagrad_apply_merged_pair": ["adagrad_apply_merged"],
    "kge_route_fill": ["route"],
    "kge_route_build": ["route"],
    "kge_route_build_group": ["route"],
    "kge_gather_rows_req": ["route"],
    "kge_gather_rows_sharded": ["gather_rows_sharded"],
    # test support
    "kge_debug_epoch_order": ["debug_epoch_order"],
}


def cases_of(name):
    v = STREAM_ENTRIES[name]
    return [] if isinstance(v, Exempt) else list(v)


def entries_of(case):
    return sorted(n for n in STREAM_ENTRIES if case in cases_of(n))


# ---- reading C ------------------------------------------------------------------------------------------------------------------
def blank_comments_and_strings(text):
    """comments, string and character literals replaced by blanks of the same length (line breaks kept): offsets, line numbers and
    parentheses outside of them are those of the file"""
    out, i, n = list(text), 0, len(text)

    def blank(a, b):
        for k in range(a, b):
            if out[k] != "\n":
                out[k] = " "
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = i
            while True:                                   # (a line comment ending in a backslash continues)
                e = text.find("\n", j)
                e = n if e < 0 else e
                if e < n and text[e - 1] == "\\":
                    j = e + 1
                    continue
                break
            blank(i, e)
            i = e
        elif text.startswith("/*", i):
            e = text.find("*/", i + 2)
            e = n if e < 0 else e + 2
            blank(i, e)
            i = e
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            blank(i + 1, min(j, n))                       # (the quotes stay: `extern "C"` is still recognisable as `extern " "`)
            i = j + 1
        else:
            i += 1
    return "".join(out)


def cut_timeline_blocks(text):
    """the lines between `#ifdef KGE_TIMELINE` (or `#if defined(KGE_TIMELINE) ...`) and its `#else` / `#endif` blanked: the developer
    timeline is compiled out of the product library.  Returns (text, number of blocks cut)"""
    lines, depth, cut_at, cuts = text.split("\n"), 0, None, 0
    for k, ln in enumerate(lines):
        s = ln.strip()
        opens = re.match(r"#\s*(if|ifdef|ifndef)\b", s)
        if cut_at is None:
            if opens and re.match(r"#\s*(ifdef\s+KGE_TIMELINE\b|if\s+defined\s*\(\s*KGE_TIMELINE\s*\))", s):
                cut_at, depth, cuts = k, 0, cuts + 1
            continue
        if opens:
            depth += 1
        elif re.match(r"#\s*endif\b", s):
            if depth == 0:
                cut_at = None
                continue
            depth -= 1
        elif re.match(r"#\s*(else|elif)\b", s) and depth == 0:
            cut_at = None
            continue
        lines[k] = ""
    assert cut_at is None, "unterminated #ifdef KGE_TIMELINE"
    return "\n".join(lines), cuts


def drop_preprocessor_lines(text):
    """every directive with its backslash continuations blanked (for the scans of declarations; the launch scan keeps them: the
    launch macros are #define bodies)"""
    lines, k = text.split("\n"), 0
    while k < len(lines):
        if lines[k].lstrip().startswith("#"):
            while True:
                cont = lines[k].rstrip().endswith("\\")
                lines[k] = ""
                if not cont or k + 1 >= len(lines):
                    break
                k += 1
        k += 1
    return "\n".join(lines)


def source_files():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp")))


def product_text(path_or_text, is_text=False):
    text = path_or_text if is_text else open(path_or_text).read()
    return cut_timeline_blocks(blank_comments_and_strings(text))[0]


def split_args(text, open_at):
    """the arguments of the call whose `(` is text[open_at], split at the commas of its own level ((), [] and {} nest; a template
    argument list with a comma must be in parentheses, as the preprocessor demands of a macro argument anyway); -> (args, end)"""
    assert text[open_at] == "("
    depth, args, start, i = 0, [], open_at + 1, open_at
    while i < len(text):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i])
                return [re.sub(r"\\\n", " ", a).strip() for a in args], i
        elif c == "," and depth == 1:
            args.append(text[start:i])
            start = i + 1
        i += 1
    raise AssertionError("unbalanced call at offset %d" % open_at)


def calls(text, pattern):
    """(name, args, line) of every call whose callee matches the regular expression `pattern` (as a whole word)"""
    out = []
    for m in re.finditer(r"\b(%s)\s*\(" % pattern, text):
        args, _ = split_args(text, m.end() - 1)
        out.append((m.group(1), args, text.count("\n", 0, m.start()) + 1))
    return out


FORBIDDEN_STREAMS = ("0", "nullptr", "NULL", "hipStreamDefault", "hipStreamLegacy", "hipStreamPerThread")


def stream_argument_ok(arg):
    """an identifier or a (hipStream_t) cast of one - and none of the names of the null / legacy / per-thread streams"""
    m = re.match(r"^(?:\(\s*hipStream_t\s*\)\s*)?([A-Za-z_]\w*)$", arg.strip())
    return bool(m) and m.group(1) not in FORBIDDEN_STREAMS


def launch_findings(text):
    """(number of hipLaunchKernelGGL calls parsed, [(line, what)] of the launches and hip*Async calls that do not name a stream)"""
    bad, launches = [], calls(text, "hipLaunchKernelGGL")
    for _, args, line in launches:
        if len(args) < 5 or not stream_argument_ok(args[4]):
            bad.append((line, "hipLaunchKernelGGL with stream argument %r" % (args[4] if len(args) > 4 else None,)))
    for name, args, line in calls(text, r"hip\w+Async"):
        if not args or not stream_argument_ok(args[-1]):
            bad.append((line, "%s with last argument %r" % (name, args[-1] if args else None)))
    return len(launches), bad


SYNC_OR_ALLOC = r"hipMemcpy|hipMemset|hipMemsetD8|hipMemsetD16|hipMemsetD32|hipMalloc\w*|hipFree\w*|hipDeviceSynchronize|" \
                r"hipStreamSynchronize|hipEventSynchronize|hipMemcpyToSymbol"


def function_bodies(text, name_pattern):
    """[(start, end)] offsets of the bodies of the functions defined at any scope whose name matches: `name(...) {` ... `}`"""
    out = []
    for m in re.finditer(r"\b(%s)\s*\(" % name_pattern, text):
        _, close = split_args(text, m.end() - 1)
        rest = re.match(r"\s*\{", text[close + 1:])
        if not rest:
            continue                                  # a call or a prototype
        i, depth = close + 1 + rest.end() - 1, 0
        start = i
        while i < len(text):
            depth += text[i] == "{"
            depth -= text[i] == "}"
            if depth == 0:
                break
            i += 1
        out.append((start, i + 1))
    return out


def sync_findings(text):
    """[(line, call)] of the synchronous / allocating runtime calls outside the bodies of the kge_ipc_* functions"""
    skip = function_bodies(text, r"kge_ipc_\w+")
    out = []
    for m in re.finditer(r"\b(%s)\s*\(" % SYNC_OR_ALLOC, text):
        if not any(a <= m.start() < b for a, b in skip):
            out.append((text.count("\n", 0, m.start()) + 1, m.group(1)))
    return out


def namespace_scope_statements(text):
    """(line, statement) of everything declared outside of function bodies: walks the braces, entering those of `namespace ... {`
    and `extern "C" {`; an initialiser's `= {...}` and the body of a struct / union / class / enum stay in their statement as `{}`
    (`struct {...} name;` declares `name`), every other body - a function's - ends its declaration"""
    text = drop_preprocessor_lines(text)
    out, i, n, cur = [], 0, len(text), []

    def skip_braces(j):
        depth = 0
        while j < n:
            depth += text[j] == "{"
            depth -= text[j] == "}"
            j += 1
            if depth == 0:
                return j
        raise AssertionError("unbalanced braces")
    while i < n:
        c = text[i]
        if c == ";":
            s = " ".join("".join(cur).split())
            del cur[:]
            if s:
                out.append((text.count("\n", 0, i) + 1, s))
        elif c == "{":
            head = " ".join("".join(cur).split())
            if re.match(r"^(inline )?namespace\b[\w :]*$", head) or re.match(r'^extern ?" *"$', head):
                del cur[:]                            # a scope: its content is namespace scope too
            else:
                i = skip_braces(i)
                if head.endswith("=") or re.search(r"\b(struct|union|class|enum)\b[\w :]*$", head) and "(" not in head:
                    cur.append(" {} ")
                else:
                    del cur[:]
                continue
        elif c == "}":
            del cur[:]                                # the end of a scope
        else:
            cur.append(c)
        i += 1
    return out


NOT_DATA = r"^(typedef|using|static_assert|template|friend|namespace)\b"
TYPE_ONLY = r"^(struct|union|class|enum)( class)? ?\w*( ?:[^{]*)? ?(\{\})?$"


def is_data(stmt):
    """a declaration of an object (not a function prototype, a type, an alias or an assertion)"""
    if re.match(NOT_DATA, stmt) or re.match(TYPE_ONLY, stmt):
        return False
    decl = re.sub(r"\b(alignas|__attribute__|__align__) ?\(\(?[^()]*\)?\)", " ", stmt.split("=")[0])
    return "(" not in decl and bool(re.search(r"\w", decl))


def state_findings(text):
    """[(line, what, statement)]: a __device__ / __constant__ variable at namespace scope; namespace-scope data (static or not) that
    is neither const / constexpr nor thread_local"""
    out = []
    for line, s in namespace_scope_statements(text):
        if not is_data(s):
            continue
        if re.search(r"\b(__device__|__constant__|__managed__)\b", s):
            out.append((line, "device-side variable at namespace scope", s))
        elif not re.search(r"\b(const|constexpr|thread_local)\b", s.split("=")[0]):
            out.append((line, "mutable data at file scope", s))
    return out


# ---- reading the header ------------------------------------------------------------------------------------------------------
def prototypes(header_text):
    """{name: [parameter, ...]} of every `kge_*` function the header declares"""
    text = drop_preprocessor_lines(blank_comments_and_strings(header_text))
    out = {}
    for line, s in namespace_scope_statements(text):
        m = re.match(r"^[\w\s\*]*?\b(kge_\w+)\s*\((.*)\)$", s)
        if m and not re.match(NOT_DATA, s):
            out[m.group(1)] = [p.strip() for p in m.group(2).split(",")]
    return out


STREAM_PARAM = r"^void\s*\*\s*(?:\w+_)?stream$"        # `void *stream`, `void *hip_stream`: any name that is or ends in _stream
STREAM_NAME = r"(?:\b|_)stream$"


def is_stream_param(param):
    return bool(re.match(STREAM_PARAM, param.strip()))


def stream_functions(protos):
    return {n: p for n, p in protos.items() if any(is_stream_param(x) for x in p)}


def workspace_functions(protos):
    """{name: index of `ws`} of every prototype with the adjacent parameters `void *ws, size_t ws_bytes`"""
    out = {}
    for n, p in protos.items():
        at = [i for i in range(len(p) - 1) if re.match(r"^void\s*\*\s*ws$", p[i]) and re.match(r"^size_t\s+ws_bytes$", p[i + 1])]
        assert len(at) <= 1, n
        if at:
            out[n] = at[0]
    return out
