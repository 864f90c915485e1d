"""Inventory guard (CPU) for the bounds tests: every declaration in include/lanemap_hip.h that takes a `void* stream` (a device launch) is
named in tests/test_gpu_1_bounds.py outside its BOUNDS_EXEMPT dict, or is a key of that dict with a non-empty reason.  A new kernel
cannot land without a guarded-buffer case or a written reason."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_FILE = os.path.join(ROOT, 'tests', 'test_gpu_1_bounds.py')


def _stream_entries():
    text = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return sorted(set(re.findall(r'\b(lm_\w+)\s*\(\s*void\s*\*\s*stream\b', text)))


def _exempt_and_body():
    src = open(GPU_FILE).read()
    tree = ast.parse(src)
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == 'BOUNDS_EXEMPT' for t in node.targets):
            seg = ast.get_source_segment(src, node)
            return ast.literal_eval(node.value), src.replace(seg, '')
    raise AssertionError('tests/test_gpu_1_bounds.py has no BOUNDS_EXEMPT dict')


def test_header_stream_entries_parse():
    names = _stream_entries()
    assert len(names) > 50 and 'lm_conv2d_nhwc_mfma_f32' in names and 'lm_las_decode_points' in names
    assert 'lm_winograd44_supported' not in names and 'lm_endp_cluster' not in names     # queries and host code take no stream


def test_every_stream_entry_has_a_bounds_case_or_reason():
    exempt, body = _exempt_and_body()
    names = _stream_entries()
    missing = [n for n in names if n not in exempt and not re.search(r'\b' + n + r'\b', body)]
    assert not missing, f'device entry points with neither a case in test_gpu_1_bounds.py nor a reason in BOUNDS_EXEMPT: {missing}'
    empty = [n for n, why in exempt.items() if not (isinstance(why, str) and why.strip())]
    assert not empty, f'BOUNDS_EXEMPT entries without a reason: {empty}'
    unknown = sorted(set(exempt) - set(names))
    assert not unknown, f'BOUNDS_EXEMPT names no stream-taking declaration of include/lanemap_hip.h: {unknown}'
    both = [n for n in exempt if re.search(r'\b' + n + r'\b', body)]
    assert not both, f'covered by a case but still exempted: {both}'
