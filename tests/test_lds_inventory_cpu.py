"""Inventory guard (CPU) for the LDS-state tests: every `__global__` function of lanemapping_amd/csrc/*.hip whose body declares
`__shared__` memory (static or extern) is a key of LDS_KERNELS in tests/test_gpu_lds_state.py - the case that runs it after poisoned
LDS - or a key of LDS_EXEMPT with one of the two accepted reasons.  A new LDS kernel cannot land without such a case."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'lanemapping_amd', 'csrc')
GPU_FILE = os.path.join(ROOT, 'tests', 'test_gpu_lds_state.py')

TWIN_REASON = 'alternative kernel behind a test-only environment switch, compared bit for bit with the default one'
SECOND_REASON = re.compile(r'reached only as the second kernel of entry lm_\w+$')


def _strip_comments(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return re.sub(r'//[^\n]*', ' ', text)


def _match(text, i, open_, close):
    """Index just past the bracket that closes the one at text[i]."""
    depth = 0
    for j in range(i, len(text)):
        if text[j] == open_:
            depth += 1
        elif text[j] == close:
            depth -= 1
            if depth == 0:
                return j + 1
    raise AssertionError('unbalanced brackets in a kernel source')


def lds_kernels(text):
    """Names of the __global__ functions of one source whose body declares __shared__ memory."""
    text = _strip_comments(text)
    out = []
    for m in re.finditer(r'\b__global__\b', text):
        h = re.compile(r'\bvoid\s+(\w+)\s*\(').search(text, m.end())
        assert h, 'a __global__ without a void function after it'
        args_end = _match(text, h.end() - 1, '(', ')')
        brace = text.index('{', args_end)
        if ';' in text[args_end:brace]:
            continue                                         # a declaration only
        body = text[brace:_match(text, brace, '{', '}')]
        if re.search(r'\b__shared__\b', body):
            out.append(h.group(1))
    return out


def _all_lds_kernels():
    names = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith('.hip'):
            for k in lds_kernels(open(os.path.join(CSRC, f)).read()):
                names.setdefault(k, f)
    return names


def _tables():
    src = open(GPU_FILE).read()
    got = {}
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Name) and t.id in ('LDS_KERNELS', 'LDS_EXEMPT'):
                    got[t.id] = ast.literal_eval(node.value)
    assert set(got) == {'LDS_KERNELS', 'LDS_EXEMPT'}, 'tests/test_gpu_lds_state.py needs literal LDS_KERNELS and LDS_EXEMPT dicts'
    return got['LDS_KERNELS'], got['LDS_EXEMPT']


def test_parser_finds_static_extern_and_template_kernels():
    names = _all_lds_kernels()
    assert len(names) > 30
    for k in ('conv_mfma_kernel', 'wino44_kernel', 'stem_mfma_kernel', 'head_stage2_lds_kernel', 'las_label_kernel', 'attention_flash_kernel'):
        assert k in names, k
    assert 'head_tokens_kernel' not in names and 'label_points_kernel' not in names      # __global__ without LDS
    dummy = '__global__ void plain(float* y) { y[0] = 1.f; }\n' \
            'template <int N> __global__ __launch_bounds__(64) void fresh_lds_kernel(float* y) { __shared__ float s[N]; y[0] = s[0]; }\n' \
            '__global__ void dyn(float* y) { extern __shared__ float d[]; y[0] = d[0]; }  // __shared__ in a comment of plain() is nothing\n'
    assert lds_kernels(dummy) == ['fresh_lds_kernel', 'dyn']


def test_every_lds_kernel_has_a_case_or_reason():
    names = _all_lds_kernels()
    cases, exempt = _tables()
    missing = sorted(k for k in names if k not in cases and k not in exempt)
    assert not missing, f'kernels with LDS and neither a case in LDS_KERNELS nor a reason in LDS_EXEMPT: {[(k, names[k]) for k in missing]}'
    unknown = sorted((set(cases) | set(exempt)) - set(names))
    assert not unknown, f'LDS_KERNELS / LDS_EXEMPT name no __global__ with __shared__ in lanemapping_amd/csrc: {unknown}'
    both = sorted(set(cases) & set(exempt))
    assert not both, f'covered by a case but still exempted: {both}'
    bad = sorted(k for k, why in exempt.items() if not (isinstance(why, str) and (why == TWIN_REASON or SECOND_REASON.match(why))))
    assert not bad, f'LDS_EXEMPT reasons other than the two accepted ones: {bad}'


def _module_functions(path):
    src = open(path).read()
    return {n.name: ast.get_source_segment(src, n) for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}


def _runs_after_poisoned_lds(funcs, name):
    """The test's body, or that of a function of its file that it calls (transitively), goes through guarded_runs, lds_state_runs or
    poisoned."""
    seen, todo = set(), [name]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        if re.search(r'\b(guarded_runs|lds_state_runs|poisoned)\s*\(', funcs[f]):
            return True
        todo += [g for g in funcs if g not in seen and re.search(r'\b' + re.escape(g) + r'\s*\(', funcs[f])]
    return False


def test_every_case_id_names_a_test_that_runs_after_poisoned_lds():
    """A case id is `file.py::test_name` (no parameter part: nothing could check it): the file is in tests/, defines that test, and the
    test goes through guarded_runs, lds_state_runs or poisoned - so a case that poisons nothing cannot stand for a kernel."""
    cases, _ = _tables()
    bad = []
    for k, ids in cases.items():
        for cid in ([ids] if isinstance(ids, str) else ids):
            f, _, t = cid.partition('::')
            path = os.path.join(ROOT, 'tests', f)
            funcs = _module_functions(path) if os.path.exists(path) else {}
            if not (re.fullmatch(r'test_\w+', t) and t in funcs and _runs_after_poisoned_lds(funcs, t)):
                bad.append((k, cid))
    assert not bad, f'LDS_KERNELS case ids that name no test, or a test that runs nothing after poisoned LDS: {bad}'


def test_the_case_check_sees_through_helpers_and_refuses_a_plain_test():
    funcs = {'test_a': 'def test_a(dev):\n    _case(dev, 1)', '_case': 'def _case(dev, n):\n    guarded_runs(run, "x")',
             'test_b': 'def test_b(dev):\n    L = lib()\n    L.lm_strip_bin_points(stream)', 'test_c': 'def test_c():\n    with lds_state.poisoned(w):\n        pass'}
    assert _runs_after_poisoned_lds(funcs, 'test_a') and _runs_after_poisoned_lds(funcs, 'test_c') and not _runs_after_poisoned_lds(funcs, 'test_b')
