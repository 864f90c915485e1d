"""GPU tests (-m gpu), file 4 of 4: every test that launches `bench.py` as a subprocess.  These assert what a test ASKED for on the
command line, never a default of bench.py (round 4's red suite was one such assertion)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from gpu_common import ROOT, _close, _lidar_module, _rowref_head
from lanemapping_amd import synth

pytestmark = pytest.mark.gpu


def test_bench_plain_command(dev):
    """The driver's plain command line (`python bench.py` with its defaults, shortened) prints ONE JSON line with the contract's keys for
    the headline workload and runs nothing the headline does not need: no CPU baseline, no second line, no checker legs (`--full` runs
    them).  What it spends outside its steps - set-up, priming batch, teardown - stays within 30 s."""
    import json
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '2', '--warmup', '1'],
                       capture_output=True, text=True, timeout=900, cwd=root)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().split('\n') if l.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert 'LAS points' in d['metric'] and d['unit'] == 'tiles/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['steps'] == 2 and d['warmup'] == 1 and d['n_gpus'] == 1 and d['value'] > 10
    assert abs(d['ms_per_step'] - 1e3 * d['config']['tiles_per_step_per_gpu'] / d['value']) < 1e-6 * d['ms_per_step']
    assert d['cpu_baseline'] is None and 'second_line' not in d
    assert d['config']['raster_check'].startswith('not run') and not d['config']['stream_check'].startswith('lanes and endpoints')
    outside = wall - (d['steps'] + d['warmup']) * d['ms_per_step'] * 1e-3
    assert outside <= 30.0, f'{outside:.1f} s outside the warm-up and timed steps'


def test_bench_default_command(dev):
    """The driver's full command line (`python bench.py --full` with its defaults, shortened) prints ONE JSON line with the contract's
    keys: the headline workload (BASELINE configs[2]: LAS points -> polylines, batch 16), a roofline whose fraction is the EXECUTED
    MFMA view (<= 1), the raster's HBM roofline, the bitwise multi-stream check and the CPU baseline."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '2', '--warmup', '1', '--full', '--cpu-budget-s', '3'],
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().split('\n') if l.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert 'LAS points' in d['metric'] and 'batch=16' in d['config']['workload'] and d['config']['tiles_per_step_per_gpu'] == 16
    assert d['steps'] == 2 and d['n_gpus'] == 1 and d['value'] > 10
    assert d['config']['stream_check'].startswith('lanes and endpoints'), d['config']['stream_check']
    rf = d['roofline']
    f44 = os.environ.get('LANEMAP_WINO_F44', '1') != '0'                 # (the suite itself may run under the switch)
    assert {'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'algorithmic_equiv_tflops', 'per_kernel'} <= set(rf)
    assert 0.0 < rf['frac'] <= 1.0 and abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-9
    assert rf['algorithmic_equiv_tflops'] >= rf['achieved'] and abs(rf['frac_survey_8d'] - rf['algorithmic_equiv_tflops'] / rf['peak']) < 1e-9
    assert all(0.0 <= v['frac'] <= 1.0 for v in rf['per_kernel'].values())
    rr = d['raster_roofline']
    # frac = the bytes the design moves (u8 tile); frac_survey_8d = SURVEY 8(d)'s numerator (f32 tile): same time, more bytes
    assert rr['bound'] == 'hbm' and 0.1 < rr['frac'] < 1.0 and rr['frac'] < rr['frac_survey_8d'] < 1.0
    assert abs(rr['frac'] - rr['achieved'] / rr['peak']) < 1e-9
    assert {'value', 'unit', 'cores', 'kind', 'sample'} <= set(d['cpu_baseline']) and d['cpu_baseline']['value'] > 0
    # the headline is exact fp32; the declared second line (fp16 x 2 split Winograd products, a child run of the same command) rides along
    assert d['dtype'] == 'f32'
    sl = d['second_line']
    assert 'error' not in sl and sl['value'] > 10 and sl['steps'] == 10 and 'NOT bit-identical' in sl['what'] and sl['dtype'] != 'f32'
    assert sl['stream_check'].startswith('lanes and endpoints') and sl['raster_check'].startswith('tiles 0 and 15')
    if f44:
        assert any('split' in k for k in sl['roofline']['per_kernel']) and 0.0 < sl['roofline']['frac'] <= 1.0
    assert (rf['winograd_ms_per_step'] > 0) == f44 and ('wino44_kernel' in rf['per_kernel']) == f44


def test_bench_self_launch_two_ranks(dev):
    """`python bench.py --gpus 2` WITHOUT a launcher spawns its two ranks itself (before touching the GPU) and prints one line
    with n_gpus 2 (both ranks share this box's single GPU over gloo through the test hooks)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env.update(LANEMAP_BENCH_DEVICE='0', LANEMAP_BENCH_BACKEND='gloo')
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--workload', 'tiles', '--steps', '2', '--warmup', '1',
                        '--full', '--cpu-budget-s', '6'], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.strip().split('\n') if l.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['config']['tiles_per_step_per_gpu'] == 8 and d['value'] > 10
    # the bench validated the CONTENT of its last all-gather on every rank (it exits non-zero otherwise): 2 x 8 valid tiles in ONE
    # byte block, each rank's slice bitwise the block it sent and equal to the lanes / endpoints of its last batch
    assert d['config']['gather_check'].startswith('last all-gather: 16 valid tiles in one [16, 169992] byte block'), d['config']['gather_check']
    # ... and the CPU path is timed on this host next to the N > 1 number too
    assert d['cpu_baseline'] is not None and d['cpu_baseline']['value'] > 0 and d['cpu_baseline']['cores'] >= 1


def test_bench_two_ranks_code_path(dev):
    """The N>1 path of bench.py (torch.distributed.run, per-rank shards, barrier + max-over-ranks timing, one all-gather of
    the polyline blocks per batch on the side stream) with two ranks sharing this box's single GPU over gloo; on the 8-GPU
    node the same code runs one rank per GPU over RCCL."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, LANEMAP_BENCH_DEVICE='0', LANEMAP_BENCH_BACKEND='gloo')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(port), os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--full',
                        '--cpu-budget-s', '6'],
                       capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.strip().split('\n') if l.startswith('{')]
    assert len(lines) == 1                                           # rank 0 only
    d = json.loads(lines[0])
    # (N > 1 lines carry the CPU baseline too: north_star wants it timed on the node's own host cores in the same run)
    assert d['n_gpus'] == 2 and d['steps'] == 3 and d['cpu_baseline'] is not None and d['cpu_baseline']['value'] > 0 and d['value'] > 10
    assert d['config']['gather_check'].startswith('last all-gather: 32 valid tiles in one [32, 169992] byte block')
    # several ranks on a node split its host cores (no --host-cores given): each took its slice; the CPU baseline ran on all of them
    assert d['config']['host_cores_auto'] is True and d['config']['host_cores_pinned'] is True
    assert d['config']['host_cores_per_rank'] <= 8 and d['cpu_baseline']['cores'] >= d['config']['host_cores_per_rank']
    assert d['config']['raster_check'].startswith('tiles 0 and 15 of the last timed 16 x 4194304-point launch equal oracle/raster_ref.c')


def test_bench_four_ranks_on_one_gpu(dev):
    """Readiness of the multi-GPU lines beyond two ranks (no multi-GPU node is available to the builder): `bench.py --gpus 4 --workload
    tiles` with FOUR ranks sharing this box's GPU over gloo - the code path the driver runs one rank per GPU over RCCL.  (Four, not the
    node's eight: with this test process, eight ranks would put nine processes on one shared GPU.)  Every rank takes its slice of the
    host cores by itself (usable cores / 4, HIP graphs on), the slices are disjoint, ONE all-gather per batch delivers 4 x 8 valid tiles
    to every rank, rank 0 prints the only line (with the CPU baseline measured while the other ranks are parked)."""
    import json
    import socket
    import subprocess
    import sys
    import bench as bench_mod
    n = 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, LANEMAP_BENCH_DEVICE='0', LANEMAP_BENCH_BACKEND='gloo')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
                        '--master-port', str(port), os.path.join(root, 'bench.py'), '--gpus', str(n), '--workload', 'tiles', '--steps', '2',
                        '--warmup', '1', '--full', '--cpu-budget-s', '4'], capture_output=True, text=True, timeout=1500, cwd=root, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.strip().split('\n') if l.startswith('{')]
    assert len(lines) == 1                                           # rank 0 only
    d = json.loads(lines[0])
    assert d['n_gpus'] == n and d['steps'] == 2 and d['scaling'] == 'weak' and d['value'] > 10
    assert d['config']['gather_check'].startswith(f'last all-gather: {n * 8} valid tiles in one [{n * 8}, 169992] byte block'), d['config']['gather_check']
    cores = bench_mod.usable_cores()
    if cores // n <= 8:              # the ranks split the node's cores
        assert d['config']['host_cores_auto'] is True and d['config']['host_cores_pinned'] is True
        assert d['config']['host_cores_per_rank'] == max(1, cores // n)
        assert d['config']['hip_graphs'] is True                     # (the default of the capturable workloads since round 5)
        allowed = sorted(os.sched_getaffinity(0))
        slices = [bench_mod.host_budget(n, n, lr, cores, allowed, None, False, 'tiles')['cores'] for lr in range(n)]
        if n * (cores // n) <= len(allowed):
            flat = [c for sl in slices for c in sl]
            assert len(flat) == len(set(flat)) == n * max(1, cores // n)          # disjoint
    assert d['cpu_baseline'] is not None and d['cpu_baseline']['value'] > 0 and f'{n - 1} other rank(s)' in d['cpu_baseline']['measured_with']


@pytest.mark.parametrize('workload', ['tiles', 'rowref', 'lidar'])
def test_bench_other_workloads(dev, workload):
    """`bench.py --workload tiles` (BASELINE configs[1]), `rowref` (configs[3]) and `lidar` (configs[4]) run and print a contract line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--workload', workload, '--steps', '2', '--warmup', '1',
                        '--full', '--no-cpu-baseline'], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.strip().split('\n') if l.startswith('{')][-1])
    assert d['value'] > 10 and 0.0 < d['roofline']['frac'] <= 1.0 and d['config']['tiles_per_step_per_gpu'] == 8


def test_bench_hip_graphs_four_streams(dev):
    """`bench.py --graphs`: four HIP graphs (one per stream / sub-batch) replayed concurrently; the bench's own check compares the last
    timed step bitwise with a kernel-by-kernel single-stream run (it raises SystemExit on any difference)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--workload', 'tiles', '--graphs', '--streams', '4', '--steps', '3', '--warmup', '1',
                        '--full', '--no-cpu-baseline'], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.strip().split('\n') if l.startswith('{')][-1])
    assert d['value'] > 10 and d['config']['hip_graphs'] is True and d['config']['streams'] == 4
    assert 'bitwise equal' in d['config']['stream_check'] and 0.0 < d['roofline']['frac'] <= 1.0


def test_bench_dump_outputs(dev, net, tmp_path):
    """`bench.py --dump-outputs DIR`: the lanes and kept endpoints of the last timed step (tiles workload: tile seeds 2021..2028, weight
    seed 2021 - the `net` fixture) are, bit for bit, what TilePipeline returns for the same tiles in this process."""
    import json
    import subprocess
    import sys
    from lanemapping_amd.pipeline import TilePipeline
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--workload', 'tiles', '--steps', '3', '--warmup', '1', '--no-cpu-baseline',
                        '--dump-outputs', str(out)], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.strip().split('\n') if l.startswith('{')][-1])
    assert d['steps'] == 3 and abs(d['ms_per_step'] - 1e3 * 8 / d['value']) < 1e-6 * d['ms_per_step']
    got = {n: np.load(out / f'{n}.npy') for n in ('lanes', 'endpoints', 'tiles')}
    assert sorted(os.listdir(out)) == ['endpoints.npy', 'lanes.npy', 'tiles.npy'] and all(a.dtype == np.float64 for a in got.values())
    want = TilePipeline(net).run_batch(torch.from_numpy(synth.bev_batch([2021 + i for i in range(8)], 1152)).to(dev))
    assert np.array_equal(got['tiles'], np.arange(8)) and np.array_equal(got['lanes'], np.stack([l for l, _ in want]))
    want_e = np.concatenate([np.concatenate([np.full((len(e), 1), t), np.asarray(e).reshape(-1, 2)], axis=1) for t, (_, e) in enumerate(want)])
    assert np.array_equal(got['endpoints'], want_e)


@pytest.mark.parametrize('points', ['host', 'las'])
def test_bench_input_inclusive_variants(dev, points):
    """`bench.py --points host` / `--points las`: the headline step with its 16 x 4,194,304 points arriving from PINNED HOST memory every
    step (double-buffered upload on a copy stream; `las`: raw LAS format-0 records, decoded on the GPU in front of the raster).  The line
    names the source, reports the upload's achieved rate, a resident-points window of the same run and the ratio, and the bench's own
    checks ran on the uploaded data (raster of the last step == C oracle; multi-stream == single-stream)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--points', points, '--steps', '4', '--warmup', '1', '--full',
                        '--no-cpu-baseline'],
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = json.loads([l for l in r.stdout.strip().split('\n') if l.startswith('{')][-1])
    f = d['config']['point_feed']
    per_point = {'host': 16, 'las': 20}[points]
    assert d['config']['points'] == points and 'PINNED HOST' in d['config']['workload'] and 'pinned host memory' in d['metric']
    assert f['bytes_per_step'] == 16 * 4194304 * per_point and f['uploads_timed'] >= 4 and f['h2d_GBps'] > 1.0
    assert 0.3 < f['fraction_of_resident'] < 1.2 and f['resident_window']['tiles_per_s_this_rank'] > 10 and d['value'] > 10
    assert d['config']['raster_check'].startswith('tiles 0 and 15 of the last timed 16 x 4194304-point launch equal oracle/raster_ref.c')
    assert d['config']['stream_check'].startswith('lanes and endpoints')


# ------------------------------------------------------------------------------------------------ multi-GPU lines over RCCL
# Two distinct devices are needed for the RCCL lines themselves; on a one-GPU box the same tests run the one-rank half and check that a
# two-GPU request is refused before any rank starts (no two-GPU number or file set is ever produced on one device).
def test_bench_two_real_gpus_over_rccl(dev):
    """`python bench.py --gpus 2` with the default `nccl` (= RCCL) backend and no test hooks.  Always: the 1-rank run of the same command
    prints its line (one rank, no process group, device 0).  With >= 2 GPUs (UNMEASURED ON HARDWARE until such a box runs it): two
    DISTINCT devices, the collective really was RCCL over two ranks, the gathered content was verified on every rank, and the whole-job
    rate is >= 1.8 x the 1-rank run (north_star: >= 0.9 linear).  With one GPU: `--gpus 2` exits non-zero without a result line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LANEMAP_BENCH_DEVICE', 'LANEMAP_BENCH_BACKEND')}

    def launch(n):
        return subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(n), '--steps', '20', '--warmup', '3', '--no-cpu-baseline'],
                              capture_output=True, text=True, timeout=1500, cwd=root, env=env)

    def run(n):
        r = launch(n)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        lines = [l for l in r.stdout.strip().split('\n') if l.startswith('{')]
        assert len(lines) == 1
        return json.loads(lines[0])
    one = run(1)
    assert one['n_gpus'] == 1 and one['steps'] == 20 and one['value'] > 10
    assert one['config']['dist_ranks'] == 1 and one['config']['dist_backend'] is None and one['config']['rank_devices'] == [0]
    if torch.cuda.device_count() < 2:
        r = launch(2)
        assert r.returncode != 0 and not any(l.startswith('{') for l in r.stdout.split('\n')), (r.stdout + r.stderr)[-3000:]
        assert '--gpus 2 but only 1 GPU(s) are visible' in r.stderr, r.stderr[-3000:]
        return
    two = run(2)
    assert two['n_gpus'] == 2 and two['config']['dist_ranks'] == 2 and two['config']['dist_backend'] == 'nccl' and two['config']['rccl_ranks'] == 2
    assert two['config']['gather_check'].startswith('last all-gather: 32 valid tiles in one [32, 169992] byte block'), two['config']['gather_check']
    assert two['config']['rank_devices'] == [0, 1], two['config']['rank_devices']
    print(f"1 GPU {one['value']:.1f} tiles/s, 2 GPUs over RCCL {two['value']:.1f} tiles/s: x{two['value'] / one['value']:.3f}")
    assert two['value'] >= 1.8 * one['value'], (one['value'], two['value'])


def test_runner_two_real_gpus_over_rccl(dev, synth_sd, tmp_path):
    """load_config_and_runner(path, '0,1') without the one-GPU test hook.  Always: the one-id run writes one file per tile.  With >= 2
    GPUs (UNMEASURED ON HARDWARE until a multi-GPU box runs it): one fresh process per GPU, RCCL all-gather, the files of the one-id run
    byte for byte.  With one GPU: the two-id runner is refused when it is built, before any rank process starts."""
    from PIL import Image
    from lanemapping_amd.runner import load_config_and_runner
    tiles = tmp_path / 'tiles'
    tiles.mkdir()
    for s_ in range(321, 328):
        Image.fromarray(synth.bev_tile_u8(s_, 1152)).save(tiles / f'1903{s_}_0001.png')
    src = open(os.path.join(ROOT, 'configs', 'Proj_polyline_fpn_vit_vertex_2.py')).read()
    outs = {}
    for ids in ('0', '0,1'):
        path = tmp_path / f'configs_{len(ids)}.py'
        path.write_text(src.replace("log_dir = './logs'", f"log_dir = {str(tmp_path / ('logs' + str(len(ids))))!r}"))
        if ids == '0,1' and torch.cuda.device_count() < 2:
            with pytest.raises(RuntimeError, match=r"gpus='0,1' names 2 GPUs \(device indices \[0, 1\]\) but this process sees 1"):
                load_config_and_runner(str(path), ids)
            assert len(os.listdir(outs['0'][1])) == 7
            return
        cfg, runner = load_config_and_runner(str(path), ids)
        runner.net.load_state_dict(synth_sd)
        outs[ids] = (runner.infer_lane_coordinate_endpoint_semantics(tiles=str(tiles), batch_size=2, write_lane_vertex=True), cfg.work_dirs)
        if ids == '0,1':
            assert runner.backend == 'nccl' and runner.devices == [0, 1]
    (ra, da), (rb, db) = outs['0'], outs['0,1']
    assert sorted(os.listdir(da)) == sorted(os.listdir(db)) and len(os.listdir(da)) == 7
    for n in os.listdir(da):
        assert open(os.path.join(da, n), 'rb').read() == open(os.path.join(db, n), 'rb').read(), n
