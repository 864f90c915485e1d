"""Inventory guard (CPU) for the stream tests (tests/stream_state.py, tests/test_gpu_streams.py).

Every `lm_*` entry whose first parameter is the stream has a class in STREAM_CLASS and is named by a case of CASE_ENTRIES or by a
reason in STREAM_EXEMPT.  The class is what the SOURCES say: the text of the entry's definition plus that of every non-kernel function
of lanemapping_amd/csrc it names, transitively and across files.  Text that synchronises (hipStreamSynchronize, hipDeviceSynchronize,
a synchronous hipMemcpy / hipMemset, an allocation or a free) or copies between host and device with hipMemcpyAsync makes the entry
'host', and then it must open with the capture guard LM_NO_CAPTURE; any other entry is 'async', must hold none of that and no
hipMemsetAsync either (captured memset nodes replay wrongly: lm_zero_async).  A name is resolved as the compiler of the file sees it
(several files have a helper called `launch`), and a call that looks like a project function and is not found fails the test.  No
hipLaunchKernelGGL, hipMemsetAsync or hipMemcpyAsync anywhere carries a literal 0, nullptr or NULL as its stream."""
import ast
import os
import re

from lds_state import stream_entries
from test_lds_inventory_cpu import CSRC, ROOT, _match, _strip_comments

HARNESS = os.path.join(ROOT, 'tests', 'stream_state.py')
GPU_FILE = os.path.join(ROOT, 'tests', 'test_gpu_streams.py')
_KEYWORDS = {'if', 'for', 'while', 'switch', 'catch', 'return', 'sizeof', 'alignof', 'decltype', 'static_assert', 'defined', '__attribute__',
             '__launch_bounds__', 'alignas', 'operator', 'constexpr'}
# what makes an entry 'host'
_WAITS = re.compile(r'\b(hipStreamSynchronize|hipDeviceSynchronize|hipEventSynchronize|hipMemcpy|hipMemset|hipMemcpyDtoH|hipMemcpyHtoD|hipMalloc|'
                    r'hipMallocAsync|hipHostMalloc|hipFree|hipFreeAsync|hipHostFree|hipMemcpyDtoHAsync|hipMemcpyHtoDAsync)\s*\(')
_HOST_KINDS = ('hipMemcpyHostToDevice', 'hipMemcpyDeviceToHost', 'hipMemcpyHostToHost', 'hipMemcpyDefault')
# the position of the stream among the arguments
_STREAM_ARG = {'hipLaunchKernelGGL': 4, 'hipMemsetAsync': 3, 'hipMemcpyAsync': 4}


def _literal(path, *names):
    got = {}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Name) and t.id in names:
                    got[t.id] = ast.literal_eval(node.value)
    assert set(got) == set(names), f'{os.path.basename(path)} needs literal {sorted(set(names) - set(got))}'
    return [got[n] for n in names]


def _code(text):
    """The source without comments and with the contents of its string and character literals blanked (they may hold brackets); the
    "C" of `extern "C"` stays."""
    def blank(m):
        s = m.group(0)
        return s if s == '"C"' else s[0] + ' ' * (len(s) - 2) + s[-1]
    return re.sub(r'"(?:[^"\\\n]|\\.)*"|\'(?:[^\'\\\n]|\\.)+\'', blank, _strip_comments(text))


_TRANSPARENT = re.compile(r'(?:\bnamespace(?:\s+\w+)?|\bextern\s*"C"|\b(?:struct|class)\s+(?:alignas\s*\(\s*\w+\s*\)\s*)?\w+(?:\s*:\s*[\w\s,:<>]+?)?)\s*$')


def functions(text):
    """{name: (body, is_kernel)} of the function definitions of one source (comments stripped by the caller): those at brace depth 0,
    where the braces of `namespace [name] {`, `extern "C" {` and `struct / class name {` do not count - most helpers and every kernel of
    csrc sit inside an anonymous namespace."""
    out = {}
    depth, i, last_end = 0, 0, 0
    n = len(text)
    opened = []                                 # per open brace: does it count?
    while i < n:
        c = text[i]
        if c == '{':
            solid = not (depth == 0 and _TRANSPARENT.search(text[last_end:i]))
            opened.append(solid)
            if solid:
                depth += 1
            else:
                last_end = i + 1
        elif c == '}':
            if opened.pop():
                depth -= 1
            if depth == 0:
                last_end = i + 1
        elif c == ';' and depth == 0:
            last_end = i + 1
        elif c == '(' and depth == 0:
            m = re.search(r'(\w+)\s*$', text[last_end:i])
            end = _match(text, i, '(', ')')
            tail = re.match(r'\s*(const\s*|noexcept\s*|->\s*[\w:<>\s\*&]+?)*\{', text[end:])
            if m and tail and m.group(1) not in _KEYWORDS:
                brace = end + tail.end() - 1
                close = _match(text, brace, '{', '}')
                out[m.group(1)] = (text[brace:close], bool(re.search(r'\b__global__\b', text[last_end:i])))
                i = last_end = close
                continue
            i = end
            continue
        i += 1
    return out


def loose_definitions(text):
    """A second, cruder look at the same text: every `name(...) {` at ANY depth that is no control statement.  It over-counts (it knows
    nothing of scopes) and is only used to notice what functions() lost."""
    names = set(re.findall(r'\b(\w+)\s*\((?:[^;{}()]|\((?:[^;{}()]|\([^;{}()]*\))*\))*\)\s*(?:const\s*|noexcept\s*)*\{', text))
    return names - _KEYWORDS


class Sources:
    """The functions of lanemapping_amd/csrc per file, the local includes of every file, and the resolution of a name as the compiler of
    one file would see it: the file's own definitions, then those of the headers it includes (transitively), then - for a name one of
    those headers only DECLARES, as prim.h and common.h do - the one definition another source file holds."""

    def __init__(self, texts):
        self.text = {f: _code(s) for f, s in texts.items()}
        self.funcs = {f: functions(s) for f, s in self.text.items()}
        self.includes = {f: [h for h in re.findall(r'#include\s+"([\w\.]+)"', _strip_comments(s)) if h in texts] for f, s in texts.items()}
        self.loose = set().union(*[loose_definitions(s) for s in self.text.values()]) if self.text else set()

    @classmethod
    def of_csrc(cls):
        return cls({f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.cpp', '.h'))})

    def scope(self, f):
        seen, todo = [], [f]
        while todo:
            g = todo.pop(0)
            if g not in seen:
                seen.append(g)
                todo += self.includes[g]
        return seen

    def resolve(self, f, name):
        """-> (file, body, is_kernel) or None."""
        scope = self.scope(f)
        for g in scope:
            if name in self.funcs[g]:
                return (g,) + self.funcs[g][name]
        if any(re.search(r'\b' + name + r'\s*\([^;{}]*\)\s*;', self.text[g]) for g in scope if g.endswith('.h')):
            homes = [g for g in self.funcs if not g.endswith('.h') and name in self.funcs[g]]
            assert len(homes) <= 1, f'{name}, declared in a header of {f}, is defined in {homes}'
            if homes:
                return (homes[0],) + self.funcs[homes[0]][name]
        return None

    def entry_file(self, entry):
        homes = [f for f in self.funcs if entry in self.funcs[f]]
        assert len(homes) == 1, f'{entry} is defined in {homes}'
        return homes[0]

    def reach(self, entry):
        """The entry's body and the bodies of the non-kernel functions it names, transitively, each name resolved from the file of the
        body that names it -> (text, unresolved): unresolved lists the calls `name(` / `name<...>(` (no member, no qualified name)
        of something that looks like a project function - `lm_*`, or a name the loose look finds defined somewhere in csrc - that
        resolve() did not find: a parser miss must fail the test, not shorten the text."""
        seen, todo, text, lost = set(), [(self.entry_file(entry), entry)], [], []
        while todo:
            f, name = todo.pop()
            if (f, name) in seen:
                continue
            seen.add((f, name))
            body = self.funcs[f][name][0]
            text.append(body)
            called = set(re.findall(r'(?<![\w\.:>])(\w+)\s*(?:<[^;(){}]*>)?\s*\(', body))
            for g in sorted(set(re.findall(r'\b\w+\b', body))):
                r = self.resolve(f, g)
                if r is None:
                    if g in called and g not in _KEYWORDS and (g.startswith('lm_') or g in self.loose):
                        lost.append(f'{g} (named in {name}, {f})')
                elif not r[2] and (r[0], g) not in seen:
                    todo.append((r[0], g))
        return '\n'.join(text), lost


def _calls(text, what):
    """The argument lists (split at top-level commas) of every call of `what` in text."""
    out = []
    for m in re.finditer(r'\b' + what + r'\s*\(', text):
        inner = text[m.end():_match(text, m.end() - 1, '(', ')') - 1]
        args, stack, cur = [], [], ''
        for k, c in enumerate(inner):
            if c in '([{' or (c == '<' and re.search(r'\w$', cur) and inner[k + 1:k + 2] not in (' ', '=', '<')):
                stack.append(c)                                          # ('<' straight after a name and before no space: a template list)
            elif c == '>' and stack and stack[-1] == '<':
                stack.pop()
            elif c in ')]}':
                while stack and stack.pop() == '<':                      # a '<' that was a comparison after all
                    pass
            if c == ',' and not stack:
                args.append(cur.strip())
                cur = ''
            else:
                cur += c
        out.append(args + [cur.strip()])
    return out


def waits(text):
    """Why this text may not be captured: the names of the waiting calls and host copies it holds."""
    why = sorted({m.group(1) for m in _WAITS.finditer(text)})
    for args in _calls(text, 'hipMemcpyAsync'):
        if len(args) < 5 or any(k in args[3] for k in _HOST_KINDS) or not args[3].startswith('hipMemcpy'):
            why.append(f'hipMemcpyAsync({args[3] if len(args) > 3 else "?"})')
    return why


_PLANTED = {
    'a.hip': '''
        #include "shared.h"
        namespace {
        static inline int helper(hipStream_t s, int* p) { LM_HIP(hipStreamSynchronize(s)); return 0; }   // waits, inside a namespace
        template <int N> __global__ __launch_bounds__(64) void k_kernel(float* y) { if (y) { y[0] = N; } }
        template <int BM> int launch(hipStream_t s, int* p) { hipLaunchKernelGGL(k_kernel<BM>, dim3(1), dim3(64), 0, s, (float*)p); return 0; }
        }  // namespace
        LM_API int lm_a(void* stream, int* p) { if (int e = helper((hipStream_t)stream, p)) return e; return 0; }
        LM_API int lm_b(void* stream, int* p) {
            LM_HIP(hipMemcpyAsync(p, p + 1, 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
            if (int e = lm_far((hipStream_t)stream, p)) return e;
            return launch<4>((hipStream_t)stream, p);
        }
        LM_API int lm_c(void* stream, int* p, const int* h) { LM_HIP(hipMemcpyAsync(p, h, 4, hipMemcpyHostToDevice, (hipStream_t)stream)); return 0; }
        LM_API int lm_d(void* stream, int* p) { LM_HIP(hipMemsetAsync(p, 0, 4, 0)); hipLaunchKernelGGL(k_kernel<4>, dim3(1), dim3(64), 0, nullptr, (float*)p); return 0; }
        LM_API int lm_e(void* stream, int* p) { return quiet((hipStream_t)stream, p, 4); }
    ''',
    'b.hip': '''
        #include "shared.h"
        namespace {
        int launch(hipStream_t s, int* p) { LM_HIP(hipStreamSynchronize(s)); return 0; }       // another file's `launch`: it waits
        }
        int lm_far(hipStream_t s, int* p) { return 0; }
        LM_API int lm_f(void* stream, int* p) { return launch((hipStream_t)stream, p); }
    ''',
    'shared.h': '''
        int lm_far(hipStream_t s, int* p);
        static int quiet(hipStream_t s, int* p, size_t n) { LM_HIP(hipMemsetAsync(p, 0, n, s)); return 0; }
    ''',
}


def memsets(text):
    """The memset enqueues of this text: no entry that may be captured may hold one."""
    return sorted({m.group(1) for m in re.finditer(r'\b(hipMemsetAsync|hipMemsetD8Async|hipMemsetD16Async|hipMemsetD32Async|hipMemset2DAsync|'
                                                   r'hipMemset3DAsync)\s*\(', text)})


def test_parser_and_classifier_on_planted_text():
    S = Sources(_PLANTED)
    assert set(S.funcs['a.hip']) == {'helper', 'k_kernel', 'launch', 'lm_a', 'lm_b', 'lm_c', 'lm_d', 'lm_e'}, sorted(S.funcs['a.hip'])
    assert S.funcs['a.hip']['k_kernel'][1] and not S.funcs['a.hip']['lm_b'][1] and set(S.funcs['b.hip']) == {'launch', 'lm_far', 'lm_f'}
    assert waits(S.reach('lm_a')[0]) == ['hipStreamSynchronize']                       # through a helper inside `namespace {`
    text, lost = S.reach('lm_b')                                                       # its own file's launch, and lm_far across files
    assert waits(text) == [] and not lost and 'k_kernel<BM>' in text and 'y[0] = N' not in text and memsets(text) == []
    assert waits(S.reach('lm_f')[0]) == ['hipStreamSynchronize']                       # b.hip's launch is the one that waits
    assert waits(S.reach('lm_c')[0]) == ['hipMemcpyAsync(hipMemcpyHostToDevice)']
    assert memsets(S.reach('lm_e')[0]) == ['hipMemsetAsync'] and waits(S.reach('lm_e')[0]) == []      # through a header's function
    assert [a[4] for a in _calls(S.funcs['a.hip']['launch'][0], 'hipLaunchKernelGGL')] == ['s']
    d = S.funcs['a.hip']['lm_d'][0]
    assert sorted(_null_streams(d)) == ['hipLaunchKernelGGL: nullptr', 'hipMemsetAsync: 0'] and not _null_streams(S.funcs['a.hip']['lm_b'][0])
    # a helper the strict parser cannot see (here: hidden behind a macro that opens its scope) is reported, not skipped
    hidden = Sources({'c.hip': 'OPEN_SCOPE int deep(hipStream_t s) { LM_HIP(hipStreamSynchronize(s)); return 0; } }\n'
                               'LM_API int lm_g(void* stream) { return deep((hipStream_t)stream); }'.replace('OPEN_SCOPE', 'void outer() {')})
    text, lost = hidden.reach('lm_g')
    assert waits(text) == [] and lost == ['deep (named in lm_g, c.hip)']
    text, lost = Sources({'c.hip': 'LM_API int lm_h(void* stream) { return lm_nowhere((hipStream_t)stream); }'}).reach('lm_h')
    assert lost == ['lm_nowhere (named in lm_h, c.hip)']


def test_the_parser_sees_the_helpers_inside_namespaces():
    S = Sources.of_csrc()
    kernels = [k for f in S.funcs.values() for k, v in f.items() if v[1]]
    assert len(kernels) > 80, f'{len(kernels)} kernels found in lanemapping_amd/csrc: the parser lost them'
    for f, name in (('conv_mfma.hip', 'launch'), ('conv_mfma.hip', 'conv_dispatch'), ('prim.hip', 'lm_prim_exclusive_scan_u32'),
                    ('profile.hip', 'las_profile_records'), ('common.h', 'lm_zero_async'), ('tile_points.h', 'lm_tile_ranges')):
        assert name in S.funcs[f] and not S.funcs[f][name][1], (f, name)
    assert sum('launch' in f for f in S.funcs.values()) >= 3, 'launch is a helper of several files: resolution is per file'
    assert S.resolve('ground.hip', 'lm_prim_exclusive_scan_u32')[0] == 'prim.hip' and S.resolve('strip.hip', 'lm_window_xf')[0] == 'tile_points.h'


def test_every_stream_entry_has_a_class_and_a_case_or_reason():
    (klass, exempt), (cases,) = _literal(HARNESS, 'STREAM_CLASS', 'STREAM_EXEMPT'), _literal(GPU_FILE, 'CASE_ENTRIES')
    names = stream_entries()
    assert len(names) >= 73, len(names)
    assert set(klass) == set(names), f'STREAM_CLASS: missing {sorted(names - set(klass))}, stale {sorted(set(klass) - names)}'
    assert set(klass.values()) <= {'async', 'host'}
    named = {e for es in cases.values() for e in es}
    assert named <= names, f'CASE_ENTRIES names no stream entry: {sorted(named - names)}'
    assert set(exempt) <= names, f'STREAM_EXEMPT: stale {sorted(set(exempt) - names)}'
    assert not named & set(exempt), f'covered by a case but still exempted: {sorted(named & set(exempt))}'
    missing = sorted(names - named - set(exempt))
    assert not missing, f'stream entries with neither a case in CASE_ENTRIES nor a reason in STREAM_EXEMPT: {missing}'
    assert all(isinstance(why, str) and len(why) > 20 for why in exempt.values())


def test_the_class_of_every_entry_is_what_its_source_says():
    klass, = _literal(HARNESS, 'STREAM_CLASS')
    S = Sources.of_csrc()
    bad = []
    for e in sorted(stream_entries()):
        f = S.entry_file(e)
        assert not S.funcs[f][e][1]
        text, lost = S.reach(e)
        if lost:
            bad.append(f'{e}: calls that look like project functions and were not found: {lost}')
        why = waits(text)
        if why:
            first = S.funcs[f][e][0][1:].lstrip().split(';')[0]          # the first statement of the entry itself
            if klass.get(e) != 'host':
                bad.append(f"{e}: {why} in its text, class must be 'host'")
            elif not re.match(r'LM_NO_CAPTURE\s*\(', first):
                bad.append(f'{e}: {why} in its text, but LM_NO_CAPTURE is not its first statement ({first[:60]!r})')
        elif klass.get(e) != 'async':
            bad.append(f"{e}: nothing in its text waits or copies host memory, class must be 'async'")
        elif memsets(text):
            bad.append(f'{e}: an entry that may be captured enqueues {memsets(text)}: captured memset nodes replay wrongly, zero with '
                       f'lm_zero_async (common.h)')
    assert not bad, '\n'.join(bad)
    hosts = sorted(e for e, k in klass.items() if k == 'host')
    assert hosts == ['lm_drape_vertices', 'lm_ground_select', 'lm_strip_bin_points', 'lm_tile_ground', 'lm_tile_intensity_window'], hosts


def test_the_capture_guard_asks_the_runtime_and_refuses_by_name():
    text = _strip_comments(open(os.path.join(CSRC, 'common.h')).read())
    guard = functions(text)['lm_refuse_capture'][0]
    assert 'hipStreamIsCapturing' in guard and 'hipStreamCaptureStatusNone' in guard and 'LM_ERR_ARG' in guard and '%s' in guard
    assert re.search(r'#define\s+LM_NO_CAPTURE\b[^\n]*\\\n(?:[^\n]*\\\n)*[^\n]*lm_refuse_capture', text)


def _null_streams(text):
    bad = []
    for what, pos in _STREAM_ARG.items():
        for args in _calls(text, what):
            s = args[pos] if len(args) > pos else '<missing>'
            if re.fullmatch(r'(\(\s*hipStream_t\s*\)\s*)?(0|nullptr|NULL|<missing>)', s):
                bad.append(f'{what}: {s}')
    return bad


def test_no_enqueue_names_the_null_stream():
    bad, n = [], 0
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(('.hip', '.cpp', '.h')):
            text = _strip_comments(open(os.path.join(CSRC, f)).read())
            n += sum(len(_calls(text, w)) for w in _STREAM_ARG)
            bad += [f'{f}: {b}' for b in _null_streams(text)]
    assert n > 100, f'only {n} enqueues found in lanemapping_amd/csrc: the parser lost them'
    assert not bad, f'enqueues on a literal null stream: {bad}'
