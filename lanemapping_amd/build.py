"""Build liblanemap_hip.so (gfx950) in-tree with hipcc, and beside it liblanemap_diag.so, the LDS diagnostics of the tests
(tests/hip, never linked into the product library).  `python -m lanemapping_amd.build`."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'liblanemap_hip.so')
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'lanemap_hip.h')   # csrc/common.h includes it: every source depends on it
DIAG_SRC = os.path.join(os.path.dirname(HERE), 'tests', 'hip')
DIAG_LIB = os.path.join(HERE, 'liblanemap_diag.so')
DIAG_SOURCES = ['lds_state.hip']        # same compiler and flags as SOURCES; linked with errors.cpp's helpers into a library of their own
SOURCES = ['errors.cpp', 'conv_mfma.hip', 'conv_wino44.hip', 'conv_direct.hip', 'norm_resize.hip', 'vit.hip', 'mixer.hip', 'head.hip', 'head_endpoint.hip',
           'decode.hip', 'raster.hip', 'strip.hip', 'ground.hip', 'intensity.hip', 'drape.hip', 'gapfill.hip', 'rowref.hip', 'prim.hip', 'lidar.hip', 'label.hip', 'profile.hip', 'residue.hip', 'postproc.cpp', 'backproject.cpp', 'png_reader.cpp', 'lane_json.cpp', 'merge_lines.cpp', 'skeleton.cpp']


# integer-output kernels whose fp32 index math must match the C oracle bit for bit
EXACT_FP = {'raster.hip', 'strip.hip', 'ground.hip', 'intensity.hip', 'drape.hip', 'lidar.hip', 'label.hip', 'profile.hip', 'residue.hip', 'backproject.cpp', 'merge_lines.cpp'}
# per-source extra flags.  conv_wino44.hip: the SLP vectoriser packs the Winograd transform's adds into v_pk_add_f32 plus a dozen
# v_mov shuffles per group; packed f32 VALU beside MFMAs costs issue slots (MI355X_MICROARCH.md, filler price list)
EXTRA_FLAGS = {'conv_wino44.hip': ['-fno-slp-vectorize']}


def _diag_sources():
    """The diagnostics sources that are there: the package also builds where the tests directory is another one, or absent - then the
    product library alone."""
    return [f for f in DIAG_SOURCES if os.path.exists(os.path.join(DIAG_SRC, f))]


def _stale():
    diag = _diag_sources()
    if not os.path.exists(LIB) or (diag and not os.path.exists(DIAG_LIB)):
        return True
    t = min([os.path.getmtime(LIB)] + ([os.path.getmtime(DIAG_LIB)] if diag else []))
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(DIAG_SRC, f) for f in diag] + [os.path.abspath(__file__), HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, 'build'), exist_ok=True)
    diag_objs = [os.path.join(HERE, 'build', 'errors.cpp.o')]
    diag_sources = _diag_sources()
    for src in SOURCES + diag_sources:
        diag = src in diag_sources
        obj = os.path.join(HERE, 'build', src + '.o')
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden',
               '-x', 'hip', '-c', os.path.join(DIAG_SRC if diag else CSRC, src), '-o', obj]
        if diag:
            cmd.insert(4, '-I' + CSRC)
        if src in EXACT_FP:
            cmd.insert(4, '-ffp-contract=off')
        for fl in EXTRA_FLAGS.get(src, []):
            cmd.insert(4, fl)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        (diag_objs if diag else objs).append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError(f'hipcc failed on {src}')
        if verbose and out.strip():
            sys.stderr.write(out.decode())
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
    subprocess.check_call(cmd)
    if diag_sources:
        subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', DIAG_LIB] + diag_objs)
    if verbose:
        print(f'built {LIB}' + (f' and {DIAG_LIB}' if diag_sources else ''))
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
