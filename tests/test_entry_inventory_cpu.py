"""Inventory guard (CPU): every `lm_*` entry point declared in include/lanemap_hip.h is exercised by the suite - named directly in a
tests/ file, or called from the body of a lanemapping_amd/ function that a tests/ file calls - or is listed below with the reason it
is not.  A new entry point cannot land without a test or a written reason.  Also: the kernel sources carry no compile-time build
switches."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# queries (workspace sizes, chunk / tile counts): their results size the launches that the tests do check
NOT_DIRECTLY_TESTED = {
    'lm_winograd44_tiles': 'query: Winograd tile count (profiling FLOP count in conv_wino44)',
}


def _declared():
    text = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return sorted(set(re.findall(r'\b(lm_\w+)\s*\(', text)))


def _test_sources():
    out = {}
    d = os.path.join(ROOT, 'tests')
    for dirpath, _, files in os.walk(d):
        for f in files:
            if f.endswith(('.py', '.c', '.sh')) and f != os.path.basename(__file__):
                out[os.path.join(dirpath, f)] = open(os.path.join(dirpath, f)).read()
    return out


def _package_functions():
    """{function name: source of its body} for every module-level function, method and class of lanemapping_amd/ (a class counts as
    called where its name is called; its special methods - __init__ creating a handle, __del__ freeing it - belong to it)."""
    pkg = os.path.join(ROOT, 'lanemapping_amd')
    funcs = {}
    for f in sorted(os.listdir(pkg)):
        if not f.endswith('.py'):
            continue
        src = open(os.path.join(pkg, f)).read()
        tree = ast.parse(src)
        for n in tree.body:
            if not isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                continue
            members = [(n, n.name)]
            if isinstance(n, ast.ClassDef):
                members += [(m, m.name if not m.name.startswith('__') else n.name) for m in n.body
                            if isinstance(m, (ast.FunctionDef, ast.AsyncFunctionDef))]
            for node, name in members:
                if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                    seg = ast.get_source_segment(src, node) if not isinstance(node, ast.ClassDef) else ''
                    funcs[name] = funcs.get(name, '') + '\n' + seg
    return funcs


def _calls(name, text):
    return re.search(r'\b' + re.escape(name) + r'\s*\(', text) is not None


def test_header_parses_into_entries():
    names = _declared()
    assert len(names) > 80 and 'lm_conv2d_nhwc_mfma_f32' in names and 'lm_rowref_decode' in names
    assert set(NOT_DIRECTLY_TESTED) <= set(names), sorted(set(NOT_DIRECTLY_TESTED) - set(names))


def test_every_entry_point_is_tested_or_listed():
    names = _declared()
    tests = '\n'.join(_test_sources().values())
    funcs = _package_functions()
    reached = {fn for fn in funcs if _calls(fn, tests)}        # called from tests/, then everything those bodies call, transitively
    frontier = set(reached)
    while frontier:
        body = '\n'.join(funcs[fn] for fn in frontier)
        frontier = {fn for fn in funcs if fn not in reached and _calls(fn, body)}
        reached |= frontier
    via = set(re.findall(r'\b(lm_\w+)\b', '\n'.join(funcs[fn] for fn in reached)))
    missing = [n for n in names if n not in NOT_DIRECTLY_TESTED and not re.search(r'\b' + n + r'\b', tests) and n not in via]
    assert not missing, f'entry points with neither a test nor a reason in NOT_DIRECTLY_TESTED: {missing}'
    # the exemptions are for queries only: an entry that is tested after all must leave the list
    stale = [n for n in NOT_DIRECTLY_TESTED if re.search(r'\b' + n + r'\b', tests)]
    assert not stale, f'named in tests/ but still listed as not directly tested: {stale}'


# the one build of every kernel source is the product build: no compile-time probe or ablation switch may come back.  A conditional may
# only test __HIPCC__ (host / device split of shared headers), __SSE2__ (host SIMD paths) or be a header's include guard
PREPROCESSOR_ALLOWED = {'__HIPCC__', '__SSE2__'}


def test_kernel_sources_have_no_build_switches():
    csrc = os.path.join(ROOT, 'lanemapping_amd', 'csrc')
    bad = []
    for f in sorted(os.listdir(csrc)):
        lines = open(os.path.join(csrc, f)).read().splitlines()
        for i, line in enumerate(lines):
            m = re.match(r'\s*#\s*(if|ifdef|ifndef|elif)\b(.*)', line)
            if not m:
                continue
            names = set(re.findall(r'[A-Za-z_]\w*', m.group(2).split('//')[0])) - {'defined'}
            guard = (f.endswith('.h') and m.group(1) == 'ifndef' and i + 1 < len(lines)
                     and re.match(r'\s*#\s*define\s+' + re.escape(m.group(2).strip()) + r'\s*$', lines[i + 1]))
            if not guard and not (names and names <= PREPROCESSOR_ALLOWED):
                bad.append(f'{f}:{i + 1}: {line.strip()}')
    assert not bad, f'compile-time switches in lanemapping_amd/csrc: {bad}'
