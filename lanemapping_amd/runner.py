"""Inference runner: the `test_gpu_0.py` / `Runner` entry of the reference (hot-path subset + the evaluation loop).

  load_config_and_runner(path, gpus)                 <- baseline/engine/runner.py:57-66 (log_dir + '/vis', work_dirs = log_dir/<dataset.train.type>)
  Runner.load_ckpt(path)                             <- :399-401 (strict, 'module.'-prefixed keys accepted)
  Runner.infer_lane_coordinate_endpoint_semantics()  <- :690-867, the reference's signature: the split `mode_data` (default cfg.dataset.test)
                                                        is listed the reference's way (datasets.py: <data_root>/<data_split_file>[mode] ->
                                                        <data_root>/cropped_tiff/<stem>.png), every tile -> <work_dirs>/<image_name[0:11]>.json
                                                        via save_lane_seq_2d when write_lane_vertex, and with gt_avail the loop's
                                                        coordinate / endpoint / semantic counters and its nine P / R / F1 lines
  Runner.infer_lane_coordinate()                     <- :606-687 (the K-Lane / RowRef entry, config 4: coordinate measures only)
  Runner.infer_lane_geometry_segmentation_segmentor()<- :945-1036 (Segmentor config)
  Runner.infer_las_to_map()                          <- the offline chain LAS -> BEV -> polylines -> LAS frame -> merged map
                                                        (read_las, Las2BEV, Runner, coor_img2pc.py, merge_lines.py) in one call
  Runner.infer_las_strip_to_map()                    <- the same chain from one LAS strip + a tile layout (points binned on the GPU)
Deviations, all deliberate: (1) tiles are walked SORTED by stem, not in the seeded shuffle of the reference's test list (SURVEY C13;
per-tile results and the summed counters do not depend on the order; datasets.load_datadir(shuffle_seed=cfg.seed) gives the reference's
order); (2) `mode_view=True` is accepted and ignored with one notice: the cv2 overlays (:793-822) are not results (OUT);
(3) keyword-only extras `tiles=` (explicit list / directory of PNG tiles instead of a split: no labels, so no evaluation),
`batch_size=`, `work_dirs=`.  Unknown keywords raise TypeError, an empty tile list raises ValueError.
Tiles are PNG files (load_img contract, datasets/laserlane_proposals.py:85-98): decoded on the host by the library's own PNG reader and DEFLATE decoder (png_io / csrc/inflate.h, on the host thread pool),
converted u8 -> f32/255 on the GPU (lm_tile_ingest_u8).  With torch.distributed initialised, tiles are sharded
over the ranks (lanemapping_amd/shard.py) and rank 0 writes every file after one all-gather per batch.
"""
import functools
import glob
import json
import os
import random

import numpy as np
import torch

from . import io_utils, ops, shard
from .boundary import load_config, load_reference_checkpoint
from .pipeline import TilePipeline
from .registry import build_net


def load_config_and_runner(path_config, gpus='0'):
    """baseline/engine/runner.py:57-66.  `gpus` is the reference's GPUS_EN string (test_gpu_0.py:7-9): one id -> a `Runner` on this
    process's GPU (cuda:$LOCAL_RANK, default 0; under torchrun every rank calls this with one id); several ids -> a `MultiGpuRunner`
    (runner_ranks.py) that fans every inference call out over one fresh process per listed GPU - the place of the reference's
    DataParallel(device_ids=range(cfg.gpus)) (:103-104).  A malformed list raises ValueError, more ids than visible GPUs RuntimeError."""
    from .runner_ranks import MultiGpuRunner, parse_gpus
    ids = parse_gpus(gpus)
    cfg = load_config(path_config)
    cfg.log_dir = cfg.log_dir + '/vis'
    os.makedirs(cfg.log_dir, exist_ok=True)
    cfg.work_dirs = cfg.log_dir + '/' + cfg.dataset.train.type
    os.makedirs(cfg.work_dirs, exist_ok=True)
    cfg.gpus = len(ids)
    if len(ids) > 1:
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            raise RuntimeError(f'gpus={gpus!r} inside an initialised torch.distributed job: every rank of a launcher-started job drives ONE '
                               f'GPU - pass one id per rank (the rank\'s device is cuda:$LOCAL_RANK)')
        return cfg, MultiGpuRunner(cfg, ids)
    return cfg, Runner(cfg)


EPS = 1e-16      # baseline/engine/runner.py:30


def _prf(tp, dets, dg, gts):
    """precision / recall / F1 from the loop's counters (runner.py:843-857)."""
    pre = tp / (dets + EPS)
    rec = dg / (gts + EPS)
    f1 = 2. * pre * rec / (pre + rec) if (pre + rec) > 0. else 0.
    return pre, rec, f1


# The stages of the LAS routes, in the order of their signatures: argument -> (cfg key, the options class of las_io).  Runner._las_<argument>
# (the argument, else cfg[key], else none) is generated from a row; only _las_threshold, whose default depends on the stages, is written out.
LAS_STAGES = {
    'select': ('las_select', 'PointFilter'),              # the point filter of the readers
    'ground': ('las_ground', 'GroundFilter'),             # the terrain following
    'intensity': ('las_intensity', 'IntensityStretch'),   # the intensity window
    'elevation': ('las_elevation', 'ElevationDrape'),     # the vertex heights
    'density': ('las_density', 'GapFill'),                # the gap fill
    'label': ('las_label', 'MarkingLabels'),              # the labelled LAS files
    'survey': ('las_survey', 'MarkingSurvey'),            # the marking profile
    'colour': ('las_colour', 'MarkingColour'),            # white or yellow, beside the profile
    'residue': ('las_residue', 'PaintResidue'),           # the paint no line explains
    'cross': ('las_cross', 'CrossSection'),               # cross-sections, the snapped lines
    'threshold': ('las_threshold', 'PaintThreshold'),     # the paint / asphalt threshold 'auto' asks for
    'stream': ('las_stream', 'StripStream'),              # the chunked strip route
}


class Runner:
    def __init__(self, cfg, device=None):
        self.cfg = cfg
        seed = int(cfg.get('seed', 2021))
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        self.device = torch.device(device or ('cuda:%d' % int(os.environ.get('LOCAL_RANK', 0))))
        if self.device.type == 'cuda':
            # the C library launches on the CURRENT HIP device / its current stream (ops._stream): one process drives one GPU
            torch.cuda.set_device(self.device)
        self.net = build_net(cfg).eval().to(self.device)

    def load_ckpt(self, path_ckpt):
        return load_reference_checkpoint(self.net, path_ckpt, strict=True)

    # ------------------------------------------------------------------------------------------------ input
    @staticmethod
    def list_tiles(source):
        if isinstance(source, (list, tuple)):
            return sorted(source)
        return sorted(glob.glob(os.path.join(source, '*.png')))

    def _decode_batch(self, paths, slot):
        """Host part of the tile ingest: the library's PNG reader inflates the batch on host threads into one of two pinned
        [n,H,W,C] buffers (pure C, no GIL, so it can run one batch ahead on a helper thread)."""
        from .png_io import read_png_batch, png_info
        with open(paths[0], 'rb') as f:
            h, w, c = png_info(f.read(64))
        pinned = self.__dict__.setdefault('_pinned', {})      # slot -> (pinned uint8 buffer, event of the last copy out of it)
        buf, ev = pinned.get(slot, (None, None))
        if ev is not None:
            ev.synchronize()                                   # the previous copy out of this buffer has finished
        if buf is None or tuple(buf.shape[1:]) != (h, w, c) or buf.shape[0] < len(paths):
            buf = torch.empty((len(paths), h, w, c), dtype=torch.uint8, pin_memory=self.device.type == 'cuda')
        view = buf[:len(paths)]
        read_png_batch(paths, threads=int(self.cfg.get('host_threads', 8)), out=view.numpy())
        pinned[slot] = (buf, None)
        return view

    def _to_device(self, view, slot):
        u8 = view.to(self.device, non_blocking=True)
        if self.device.type == 'cuda':
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._pinned[slot] = (self._pinned[slot][0], ev)
        if u8.shape[-1] < 3:                                   # greyscale tiles: replicate into the 3 input channels
            u8 = u8[..., :1].expand(-1, -1, -1, 3).contiguous()
        elif u8.shape[-1] > 3:                                 # RGBA: the reference keeps the first three channels (load_img)
            u8 = u8[..., :3].contiguous()
        return u8           # the stem kernel takes the u8 HWC tile and applies u8 / 255 itself (ops.stem; == ops.tile_ingest + f32 stem)

    def _load_batch(self, paths):
        return self._to_device(self._decode_batch(paths, 0), 0)

    def _batches(self, paths, B):
        """Yields the device tensor of every batch; batch i+1 is decoded on a helper thread while batch i is enqueued and runs."""
        from concurrent.futures import ThreadPoolExecutor
        chunks = [paths[i:i + B] for i in range(0, len(paths), B)]
        if not chunks:
            return
        with ThreadPoolExecutor(max_workers=1) as pool:
            fut = pool.submit(self._decode_batch, chunks[0], 0)
            for k in range(len(chunks)):
                view = fut.result()
                if k + 1 < len(chunks):
                    fut = pool.submit(self._decode_batch, chunks[k + 1], (k + 1) & 1)
                yield self._to_device(view, k & 1)

    # ------------------------------------------------------------------------------------------------ inference
    def _entries(self, mode_data, tiles):
        """The tiles of a run, sorted by stem: [(image_name, png path, dataset entry | None)]."""
        from . import datasets
        if tiles is not None:
            paths = self.list_tiles(tiles)
            ents = [(os.path.splitext(os.path.basename(p))[0][0:11], p, None) for p in paths]
        else:
            split = self.cfg.dataset.test if mode_data is None else mode_data
            ents = sorted(datasets.split_entries(split, self.cfg), key=lambda e: e['stem'])
            # the reference's stems keep the dot of '<stem>.json' (laserlane_proposals.py:534) and are cut to 11 characters (:76)
            ents = [((e['stem'] + '.')[0:11], e['image'], e) for e in ents]
        if not ents:
            raise ValueError('Runner: no tiles to process (' + (f'tiles={tiles!r}' if tiles is not None else 'the split lists none') + ')')
        missing = [p for _, p, _ in ents if not os.path.isfile(p)]
        if missing:
            raise FileNotFoundError(f'Runner: {len(missing)} of {len(ents)} tiles do not exist, first: {missing[0]}')
        return ents

    def _view_notice(self, mode_view):
        if mode_view and not self.__dict__.get('_view_noticed'):
            self._view_noticed = True
            print('lanemapping_amd.Runner: mode_view=True - the *_source / *_offset / *_seg / *_gt PNG overlays of the reference are '
                  'not produced (cv2 drawing is outside the hot path); results, JSON files and metrics are unaffected')

    def _infer(self, path_ckpt, mode_data, mode_view, gt_avail, write_lane_vertex, measures, tiles, batch_size, work_dirs):
        """Shared body of the two detector entries.  measures: subset of ('coor', 'endp', 'semantic') | ('klane',)."""
        from . import datasets, hostpost, metric_utils
        if path_ckpt:
            self.load_ckpt(path_ckpt)
        self._view_notice(mode_view)
        ents = self._entries(mode_data, tiles)
        if tiles is not None:
            gt_avail = False                                     # an explicit tile list carries no labels
        out_dir = work_dirs or self.cfg.get('work_dirs', './work_dirs')
        if write_lane_vertex:
            os.makedirs(out_dir, exist_ok=True)
        B = int(batch_size or self.cfg.get('batch_size', 8))
        dist = torch.distributed
        world = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        lo, hi, per = shard.shard_range(len(ents), rank, world)
        mine = ents[lo:hi]
        rowref = self.cfg.heads.type == 'RowSharNotReducRef'
        # ColumnProposal2 (configs 2/3/5) and RowSharNotReducRef (config 4: 12 lanes x 144 rows padded into the same [72,144,2] block)
        pipe = TilePipeline(self.net, host_threads=int(self.cfg.get('host_threads', 8)), with_decode_endp=True)
        lanes_all, endp_all = [], []
        counters = np.zeros(12, dtype=np.float64)      # coor TP / segs / DG / gts, endp TP / dets / DG / gts, semantic TP / dets / DG / gts
        buf = self.cfg.validate_buffer if gt_avail else None

        def take(futs):
            for f in futs:
                lanes, kept, pts = f.result()
                k = len(lanes_all)
                lanes_all.append(lanes); endp_all.append(kept)
                if not gt_avail:
                    continue
                gt = datasets.load_eval_gt(mine[k][2], self.cfg, merge_connect_lines=not rowref)
                if 'klane' in measures:                          # runner.py:640-651: cal_coor_measures(coor_label, cls_offset_smooth[:, :])
                    L = int(self.net.heads.num_cls)
                    label = datasets.klane_coor_label(gt['label_raw'], L, int(self.net.heads.row_size))
                    counters[0:4] += metric_utils.cal_coor_measures(label, lanes[:L, :, 0], 'conf', offset_thre=buf)[3:7]
                if 'coor' in measures:                           # :742-768
                    counters[0:4] += metric_utils.cal_coor_measures(gt['lc_coor_raw'], lanes[:, :, 0], 'conf', offset_thre=buf)[3:7]
                if 'endp' in measures:                           # :770-777: output['endp'] = the decode's endpoint map (on CUDA the
                    pred = np.zeros(gt['endp_map'].shape, dtype=np.float32)      # post-processing filters a host COPY of it)
                    if len(pts):
                        pred[pts[:, 0], pts[:, 1]] = 1.
                    counters[4:8] += metric_utils.eval_metric_endp_detector(pred, gt['endp_map'], r_thre=buf * 2)[3:7]
                if 'semantic' in measures:                       # :779-787 on lane_maps['semantic_line'] (renew_semantic_map raster)
                    counters[8:12] += metric_utils.eval_metric_line_segmentor(hostpost.raster_semantic_map(lanes), gt['mask'],
                                                                             bi_seg=False, semantics=2, buff=buf)[3:7]

        # per-tile JSON files (rank 0): written by a few helper threads - the text comes from the C library (lm_lane_json_write, no GIL) -
        # while the next batches run; a single rank starts them as the tiles complete, several ranks after the all-gather
        from concurrent.futures import ThreadPoolExecutor
        writers = ThreadPoolExecutor(max_workers=4) if (write_lane_vertex and rank == 0) else None
        writes = []

        def write_json(name, lanes):
            io_utils.save_lane_seq_2d(io_utils.pack_lane_vertices(np.asarray(lanes, dtype=np.float64)),
                                      os.path.join(out_dir, name + '.json'), with_pervertex_semantics=True)

        def take_and_write(futs):
            k0 = len(lanes_all)
            take(futs)
            if writers is not None and world == 1:
                writes.extend(writers.submit(write_json, mine[k][0], lanes_all[k]) for k in range(k0, len(lanes_all)))

        for proj in self._batches([p for _, p, _ in mine], B):
            take_and_write(pipe.submit(proj))
        take_and_write(pipe.flush())
        if world > 1:
            block = shard.pack_tile_results(lanes_all, endp_all, per, self.device)
            gathered = shard.unpack_gathered(shard.all_gather_results(block))[:len(ents)]     # ONE collective for the whole job
            names = ents
            if gt_avail:                                         # + one 96-byte all-reduce of the counters when a labelled set is scored
                t = torch.from_numpy(counters).to(self.device)
                dist.all_reduce(t)
                counters = t.cpu().numpy()
        else:
            gathered = list(zip(lanes_all, endp_all))
            names = mine
        results = {}
        for (name, _, _), (lanes, endp) in zip(names, gathered):
            results[name] = (lanes, endp)
            if writers is not None and world > 1:
                writes.append(writers.submit(write_json, name, lanes))
        if writers is not None:
            for w in writes:
                w.result()                                       # (an I/O error of any file is raised here)
            writers.shutdown()
        self.counters = counters
        return results

    def infer_lane_coordinate_endpoint_semantics(self, path_ckpt=None, mode_data=None, mode_view=False, gt_avail=True,
                                                 write_lane_vertex=False, eval_coor=True, eval_endp=True, eval_semantic=True,
                                                 *, tiles=None, batch_size=None, work_dirs=None):
        """The reference's entry (runner.py:690-867), same positional / keyword signature.  Returns {image_name: (lanes [72,144,2],
        endpoints [k,2])} (all tiles on every rank); self.metrics holds the nine numbers the reference prints, self.counters the sums."""
        measures = tuple(m for m, on in (('coor', eval_coor), ('endp', eval_endp), ('semantic', eval_semantic)) if on)
        results = self._infer(path_ckpt, mode_data, mode_view, bool(gt_avail), write_lane_vertex, measures, tiles, batch_size, work_dirs)
        c = self.counters
        zero = (0., 0., 0.)
        evaluated = bool(gt_avail) and tiles is None
        coor = _prf(*c[0:4]) if evaluated and eval_coor else zero
        endp = _prf(*c[4:8]) if evaluated and eval_endp else zero
        sem = _prf(*c[8:12]) if evaluated and eval_semantic else zero
        self.metrics = {'coordinate_prec': coor[0], 'coordinate_rec': coor[1], 'coordinate_f1': coor[2],
                        'endpoint_prec': endp[0], 'endpoint_rec': endp[1], 'endpoint_f1': endp[2],
                        'semantic_prec': sem[0], 'semantic_rec': sem[1], 'semantic_f1': sem[2]}
        if not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0:
            for k, v in self.metrics.items():                    # the reference's nine lines (:859-867)
                print(f'{k}={v}')
        return results

    def infer_lane_coordinate(self, path_ckpt=None, mode_view=False, gt_avail=True, write_lane_vertex=False,
                              *, tiles=None, batch_size=None, work_dirs=None):
        """The K-Lane / RowRef entry (runner.py:606-687; config 4): cfg.dataset.test, coordinate measures on cls_offset_smooth[:, :]."""
        results = self._infer(path_ckpt, None, mode_view, bool(gt_avail), write_lane_vertex, ('klane',), tiles, batch_size, work_dirs)
        coor = _prf(*self.counters[0:4]) if (gt_avail and tiles is None) else (0., 0., 0.)
        self.metrics = {'coordinate_prec': coor[0], 'coordinate_rec': coor[1], 'coordinate_f1': coor[2]}
        if not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0:
            for k, v in self.metrics.items():
                print(f'{k}={v}')
        return results

    def _las_option(self, arg, key, cls, value):
        """A stage of the LAS routes (`arg` of infer_las_to_map): the argument, else cfg[key] (a dict of the arguments of las_io's class
        `cls`), else none."""
        from . import las_io
        cls = getattr(las_io, cls)
        if value is None and self.cfg.get(key) is not None:
            value = cls(**dict(self.cfg.get(key)))
        if value is not None and not isinstance(value, cls):
            raise TypeError(f'{arg} must be a las_io.{cls.__name__}, not {type(value).__name__}')
        return value

    _AUTO = (('label', 'min_intensity'), ('survey', 'min_intensity'), ('cross', 'paint_intensity'), ('residue', 'min_intensity'))

    def _las_threshold(self, threshold, stages):
        """`threshold=` of the LAS routes: the argument, else cfg['las_threshold'] (a dict of las_io.PaintThreshold's arguments), else
        PaintThreshold() when a stage of `stages` ({'label': ..., 'survey': ..., 'cross': ..., 'residue': ...}) asks for 'auto', else none."""
        from . import las_io
        threshold = self._las_option('threshold', *LAS_STAGES['threshold'], threshold)
        asked = any(stages[k] is not None and getattr(stages[k], name) == las_io.AUTO for k, name in self._AUTO)
        return las_io.PaintThreshold() if threshold is None and asked else threshold

    def _las_options(self, given, las_paths):
        """What both LAS routes do with their stage arguments before anything runs.  given: {argument: value} in the order of LAS_STAGES
        (`stream` only on the strip route), each resolved by its Runner._las_<argument>, `threshold` last: its 'auto' rule reads the
        stages; then _label_plan and _colour_plan over `las_paths`.  -> ({argument: options object or None}, the `stages` of _after_map)."""
        opt = {arg: getattr(self, '_las_' + arg)(value) for arg, value in given.items() if arg != 'threshold'}
        stages = {k: opt[k] for k, _ in self._AUTO}
        opt['threshold'] = self._las_threshold(given['threshold'], stages)
        if opt['label'] is not None:
            self._label_plan(las_paths)                                    # (a basename collision is refused before anything runs)
        self._colour_plan(opt['colour'], opt['survey'], las_paths)
        return opt, stages

    def _threshold_inputs(self, threshold, stages, files, result, out_dir, chunk_records=None):
        """The stage after the merge and before `label`: the paint / asphalt histograms of the lines the call returns (the same lines as
        _survey_inputs takes) from every input file (files: (path, shift, select) in input order, a file listed several times is used
        once): one lm_las_line_hist_records call per file into one table, one read-back (las_io.hist_files).  The raw table goes to
        <out_dir>/params/paint_hist.npy ([L, Z, NB] int64), what las_io.paint_threshold reads off it to paint_threshold.json as
        {'strip': group, 'lines': {line number: group}}.  -> `stages` with every 'auto' replaced by the strip's threshold, on copies of the
        option objects.  A stage that asked for 'auto' of a strip whose group is not supported is a ValueError, raised after the files are
        written and before any stage runs.  Without lines both files are empty, and 'auto' becomes 0.0: every stage then writes its empty
        outputs whatever the number.
        threshold.scope 'line' or 'window': ONE windowed pass (las_io.hist_window_files: lm_las_line_hist_window_records, a histogram per
        station window of every line; one window per line for 'line') takes the place of the per-line pass.  The per-line table is the sum
        of its windows, so paint_hist.npy and the 'strip' and 'lines' of the JSON are computed from it and are what the strip scope writes.
        In addition: paint_hist_windows.npy ([R, Z, NB] int64), paint_table.npy (thr, source and win_start in one array:
        las_io.save_paint_table) and a 'windows' key in the JSON, {line number: [[start_m, end_m, threshold, source, supported,
        separation], ...]}, source one of 'window', 'line', 'strip'.  Every 'auto' then becomes the las_io.PaintTable (las_io.paint_table:
        a window without support takes its line's threshold, a line without support the strip's), which the stages look up per return
        on the GPU."""
        from . import las_io
        lines = self._result_lines(result)
        par_dir = self._params_dir(out_dir)
        asked = [k for k, name in self._AUTO if stages[k] is not None and getattr(stages[k], name) == las_io.AUTO]
        local = threshold.scope != 'strip'
        if local:
            hist_w, win_start, window = las_io.hist_window_files(self._each_once(files), lines, threshold, device=self.device,
                                                                 **self._chunked(chunk_records))
            hist = las_io.line_hist_of_windows(hist_w, win_start)
        else:
            hist = las_io.hist_files(self._each_once(files), lines, threshold, device=self.device, **self._chunked(chunk_records))
        found = las_io.paint_threshold(hist, threshold)
        np.save(os.path.join(par_dir, 'paint_hist.npy'), hist)
        report = {'strip': found['strip'], 'lines': {str(k): g for k, g in found['lines'].items()}}
        table = None
        if local:
            np.save(os.path.join(par_dir, 'paint_hist_windows.npy'), hist_w)
            if found['strip']['supported'] or not lines:
                table, groups = las_io.paint_table(hist_w, win_start, threshold, window)
                las_io.save_paint_table(os.path.join(par_dir, 'paint_table.npy'), table)
                report['windows'] = {str(k): [[j * window, (j + 1) * window, float(table.thr[win_start[k - 1] + j]),
                                               las_io.SOURCES[int(table.source[win_start[k - 1] + j])], g['supported'], g['separation']]
                                              for j, g in enumerate(gs)] for k, gs in groups['windows'].items()}
        with open(os.path.join(par_dir, 'paint_threshold.json'), 'w') as f:
            json.dump(report, f, indent=1)
        g = found['strip']
        if asked and lines and not g['supported']:
            raise ValueError(f"{', '.join(asked)}: 'auto' needs a threshold between asphalt and paint, and the strip's returns do not support "
                             f"one: separation {g['separation']:.4f} with {g['inner_returns']} returns on the lines and "
                             f"{g['outer_returns']} beside them (las_io.paint_threshold; {os.path.join(par_dir, 'paint_threshold.json')})")
        value = table if local else g['threshold'] if lines else 0.0
        return {k: stages[k]._replace(**{dict(self._AUTO)[k]: value}) if k in asked else stages[k] for k in stages}

    def _after_map(self, threshold, stages, colour, files, result, out_dir, chunk_records=None):
        """The stages of the LAS routes that follow the merge, in their order: threshold, label, survey (with colour), cross, residue.
        chunk_records: None, or the records every stage reads and uploads of a file at a time (`stream=` of the strip route)."""
        if threshold is not None:
            stages = self._threshold_inputs(threshold, stages, files, result, out_dir, chunk_records)
        if stages['label'] is not None:
            self._label_inputs(stages['label'], files, result, out_dir, chunk_records)
        if stages['survey'] is not None:
            self._survey_inputs(stages['survey'], files, result, out_dir, colour, chunk_records)
        if stages['cross'] is not None:
            self._cross_inputs(stages['cross'], files, result, out_dir, chunk_records)
        if stages['residue'] is not None:
            self._residue_inputs(stages['residue'], files, result, out_dir, chunk_records)

    @staticmethod
    def _chunked(chunk_records):
        """The keyword the stages after the map pass on to las_io: none without `stream=`, so that call stays what it was."""
        return {} if chunk_records is None else {'chunk_records': chunk_records}

    @staticmethod
    def _colour_plan(colour, survey, paths):
        """`colour=` is read off the survey's pass over the records: without `survey=` it is refused, and so is an input file whose point
        format carries no R, G, B (the header of every file is read here) - before anything runs."""
        from . import las_io
        if colour is None:
            return
        if survey is None:
            raise ValueError('colour: the colours are accumulated by the survey of the markings; pass survey= (a las_io.MarkingSurvey) with it')
        for path in paths:
            las_io.require_colour(path)

    @staticmethod
    def _params_dir(out_dir):
        """<out_dir>/params, made if need be: where the LAS routes record what they used."""
        par_dir = os.path.join(out_dir, 'params')
        os.makedirs(par_dir, exist_ok=True)
        return par_dir

    @staticmethod
    def _label_plan(paths):
        """The input files of a `label=` call, each once (a file listed with several parameter files is labelled once, with the first
        listing's read offset), in input order.  The outputs are named by the input's basename: two different files that share one would
        overwrite each other in labelled/ and labels.json and are refused, before anything is read."""
        seen, plan = {}, []
        for path in paths:
            real, base = os.path.realpath(path), os.path.basename(path)
            if seen.setdefault(base, real) != real:
                raise ValueError(f'label: {seen[base]} and {real} share the basename {base!r}, under which both would be written to '
                                 'labelled/; rename one of them')
            if real not in plan:
                plan.append(real)
        return plan

    @staticmethod
    def _result_lines(result):
        """The lines a LAS route returns, as the stages after the map take them: result = (lines3d, merged) -> `merged`, or the tiles' 3-D
        lines in tile-name order when nothing was merged."""
        lines3d, merged = result
        return list(merged) if len(merged) else [l for name in sorted(lines3d) for l in lines3d[name]]

    @staticmethod
    def _each_once(files):
        """files: (path, shift, select) in input order -> the same list with every real file once: a file listed several times (under
        another name too) keeps the read offset and filter of its first listing."""
        seen, once = set(), []
        for path, shift, select in files:
            if os.path.realpath(path) not in seen:
                seen.add(os.path.realpath(path))
                once.append((path, shift, select))
        return once

    def _label_inputs(self, labels, files, result, out_dir, chunk_records=None):
        """The last stage of the LAS routes: every input file (files: (path, shift, select) in input order) labelled against the lines the
        call returns - `merged`, or the tiles' 3-D lines in tile-name order when nothing was merged - and written to
        <out_dir>/labelled/<basename>; what was done goes to <out_dir>/params/labels.json as {file: [records, labelled, [per-line counts]]}."""
        from . import las_io
        lines = self._result_lines(result)
        self._label_plan([f[0] for f in files])                            # (a basename collision is refused before anything is read)
        done = {}
        for path, shift, select in self._each_once(files):
            base = os.path.basename(path)
            r = las_io.label_las(path, os.path.join(out_dir, 'labelled', base), lines, labels, shift, select=select, device=self.device,
                                 **self._chunked(chunk_records))
            done[base] = [r['records'], r['labelled'], r['per_line']]
        with open(os.path.join(self._params_dir(out_dir), 'labels.json'), 'w') as f:
            json.dump(done, f, indent=1)

    def _survey_inputs(self, survey, files, result, out_dir, colour=None, chunk_records=None):
        """The stage after `label`: the lines the call returns - `merged`, or the tiles' 3-D lines in tile-name order when nothing was
        merged - profiled from every input file (files: (path, shift, select) in input order; a file listed several times is surveyed
        once, with its first listing's read offset): one lm_las_line_profile_records call per file into one bins tensor, one read-back.
        The raw bins go to <out_dir>/params/markings.npy, what las_io.marking_summary reads off them to <out_dir>/params/markings.json
        as {line number: summary}.
        colour: a las_io.MarkingColour or None.  With one the call per file is lm_las_line_colour_records - still one pass over every file
        and one read-back -, the colour table goes to <out_dir>/params/marking_colours.npy, and every line's summary in markings.json also
        carries the keys of las_io.marking_colours.  markings.npy holds the same bytes either way."""
        from . import las_io
        lines = self._result_lines(result)
        once = self._each_once(files)
        if colour is None:
            bins, bin_start = las_io.survey_files(once, lines, survey, device=self.device, **self._chunked(chunk_records))
            summary = las_io.marking_summary(bins, bin_start, survey)
        else:
            bins, colours, bin_start = las_io.survey_colour_files(once, lines, survey, colour, device=self.device, **self._chunked(chunk_records))
            summary = [{**m, **c} for m, c in zip(las_io.marking_summary(bins, bin_start, survey),
                                                  las_io.marking_colours(bins, colours, bin_start, survey, colour))]
        par_dir = self._params_dir(out_dir)
        np.save(os.path.join(par_dir, 'markings.npy'), bins)
        if colour is not None:
            np.save(os.path.join(par_dir, 'marking_colours.npy'), colours)
        with open(os.path.join(par_dir, 'markings.json'), 'w') as f:
            json.dump({str(k + 1): m for k, m in enumerate(summary)}, f, indent=1)

    def _cross_inputs(self, cross, files, result, out_dir, chunk_records=None):
        """The stage after `survey`: the cross-section table of the lines the call returns (the same lines as _survey_inputs takes) from
        every input file (files: (path, shift, select) in input order, a file listed several times is used once): one
        lm_las_line_cross_records call per file into one table, one read-back (las_io.cross_files).  The raw table goes to
        <out_dir>/params/cross_sections.npy ([n_bins, nl, 4] int64), what las_io.cross_summary reads off it to cross_sections.json as
        {line number: summary}, and the lines moved onto their paint (las_io.snap_lines) to
        <out_dir>/out_pc_seq_json_dir/merged_snapped.txt and merged_snapped_downsample.txt, in the format of merged.txt.  Without lines
        all four are empty."""
        from . import las_io, merge_lines as ml
        lines = self._result_lines(result)
        once = self._each_once(files)
        cells, bin_start = las_io.cross_files(once, lines, cross, device=self.device, **self._chunked(chunk_records))
        summary = las_io.cross_summary(cells, bin_start, cross)
        snapped = las_io.snap_lines(lines, summary, bin_start, cross)
        par_dir = self._params_dir(out_dir)
        np.save(os.path.join(par_dir, 'cross_sections.npy'), cells)
        with open(os.path.join(par_dir, 'cross_sections.json'), 'w') as f:
            json.dump({str(k + 1): m for k, m in enumerate(summary)}, f, indent=1)
        pc_dir = os.path.join(out_dir, 'out_pc_seq_json_dir')
        os.makedirs(pc_dir, exist_ok=True)
        io_utils.save_seqs_list(snapped, os.path.join(pc_dir, 'merged_snapped.txt'))
        io_utils.save_seqs_list([ml.downsample_seqs(m) for m in snapped if m.shape[0] >= 2], os.path.join(pc_dir, 'merged_snapped_downsample.txt'))

    def _residue_inputs(self, residue, files, result, out_dir, chunk_records=None):
        """The stage after `survey` and `cross`: the paint that none of the lines the call returns explains (the same lines as _survey_inputs takes),
        from every input file (files: (path, shift, select) in input order, a file listed several times is used once): one
        ops.paint_residue call over all files, one read-back (las_io.residue_files).  The raw statistics go to
        <out_dir>/params/residue.npy ([K,12] int64), the cells to residue_cells.npy ([M,3] int32: cx, cy, component) and what
        las_io.residue_summary reads off them to residue.json as {blob number from 1: summary}.  Without lines all three are empty."""
        from . import las_io
        lines = self._result_lines(result)
        once = self._each_once(files)
        par_dir = self._params_dir(out_dir)
        if lines and once:
            blobs = las_io.residue_files(once, lines, residue, device=self.device, **self._chunked(chunk_records))
            stats = blobs.stats
            cells = np.concatenate([blobs.cells, blobs.comp[:, None]], axis=1).astype(np.int32)
            summary = las_io.residue_summary(blobs, lines, residue)
        else:
            stats, cells, summary = np.zeros((0, 12), np.int64), np.zeros((0, 3), np.int32), []
        np.save(os.path.join(par_dir, 'residue.npy'), stats)
        np.save(os.path.join(par_dir, 'residue_cells.npy'), cells)
        with open(os.path.join(par_dir, 'residue.json'), 'w') as f:
            json.dump({str(b['blob']): b for b in summary}, f, indent=1)

    def _follow_ground(self, gf, names, plist, points, offs, rpar, H, W, out_dir):
        """One batch of tiles through a las_io.GroundFilter: -> (plist, points, offs, rpar) to rasterise and back-project with.  The ground
        model comes from the batch's point ranges (ops.tile_ground); with gf.datum every tile's local_min_ele is replaced in BOTH its
        LmRasterParams (the rasteriser writes G against it) and its parameter dict (the back-projection reads z = G * ele_reso +
        local_min_ele from it); with gf.height_range the tiles are rasterised from the selected points.  The parameters actually used
        are written to <out_dir>/params/<name>.txt."""
        from . import las_io
        from ._lib import LmRasterParams
        ground, gmin = ops.tile_ground(points, offs, rpar, H, W, cell_px=gf.cell_px)
        if gf.datum:
            gmin_host = gmin.cpu().numpy()                          # the one read-back of the datum
            plist, rpar = [dict(p) for p in plist], [LmRasterParams.from_buffer_copy(r) for r in rpar]
            for j, p in enumerate(plist):
                p['local_min_ele'] = las_io.ground_datum(gmin_host[j], p['ele_reso'], gf.datum_margin, p['local_min_ele'])
                rpar[j].local_min_ele = p['local_min_ele']
        if gf.height_range is not None:
            points, offs = ops.ground_select(points, offs, rpar, ground, H, W, gf.cell_px, gf.height_range)
        par_dir = self._params_dir(out_dir)
        for name, p in zip(names, plist):
            io_utils.save_pc_2_img_transform_paras(os.path.join(par_dir, name + '.txt'), p)
        return plist, points, offs, rpar

    @staticmethod
    def _strip_intensity(st, points, offs, rpar, H, W):
        """scope='strip': the one window of all tiles of the call, from all binned ranges (one group): -> (inten_lo, inten_hi, scale, count).
        One device-to-host read."""
        from . import las_io
        window, count = ops.tile_intensity_window(points, offs, rpar, H, W, percentiles=st.percentiles, group=[0] * len(rpar))
        lo, hi, n = (int(v) for v in torch.cat([window.to(torch.int64), count[:, None]], dim=1).cpu().numpy()[0])   # the one read-back
        return (*las_io.intensity_window(lo, hi, n, st), n)

    def _balance_intensity(self, st, names, points, offs, rpar, H, W, out_dir, bal, reference=None):
        """One batch of tiles through the balance of a las_io.IntensityStretch(balance=True): the intensities of `points` in the batch's
        ranges are balanced IN PLACE (the rule: include/lanemap_hip.h).  reference: None (scope='tile': every tile's own lower median key
        and count, ops.tile_intensity_window with percentiles (50, 50), one device-to-host read) or the (key, count) of the whole call
        (scope='strip').  Then ops.tile_intensity_cells, one device-to-host read of model and count, las_io.balance_gains on the host and
        ops.tile_intensity_apply.  In place, because what reads the binned points afterwards is the window fit and the rasteriser, which
        are meant to see the balanced values, and `elevation`, which reads heights only.  `bal` collects over the call what is written
        to <out_dir>/params/balance.json as {tile name: [reference, known cells, cells, smallest gain, largest gain]} and to
        balance_gains.npy as [tiles, Gy, Gx] float32, in the order of the tiles."""
        from . import las_io
        bal = {} if bal is None else bal
        if reference is None:
            window, count = ops.tile_intensity_window(points, offs, rpar, H, W, percentiles=(50.0, 50.0))
            both = torch.cat([window[:, :1].to(torch.int64), count[:, None]], dim=1).cpu().numpy()
            ref, cnt = both[:, 0], both[:, 1]
        else:
            ref, cnt = np.full(len(rpar), int(reference[0]), np.int64), np.full(len(rpar), int(reference[1]), np.int64)
        _, count, model = ops.tile_intensity_cells(points, offs, rpar, H, W, cell_px=st.cell_px, q_ppm=500000, min_points=st.cell_min_points)
        host = torch.stack([model, count]).cpu().numpy()                    # the one read-back
        gains = las_io.balance_gains(host[0], ref, st, count=cnt)
        ops.tile_intensity_apply(points, offs, rpar, torch.from_numpy(gains).to(points.device), H, W, cell_px=st.cell_px)
        for j, name in enumerate(names):
            bal.setdefault('rows', {})[name] = [int(ref[j]), int((host[1][j] >= st.cell_min_points).sum()), int(host[1][j].size),
                                                float(gains[j].min()), float(gains[j].max())]
            bal.setdefault('gains', {})[name] = gains[j]
        par_dir = self._params_dir(out_dir)
        with open(os.path.join(par_dir, 'balance.json'), 'w') as f:
            json.dump(bal['rows'], f, indent=1)
        np.save(os.path.join(par_dir, 'balance_gains.npy'), np.stack(list(bal['gains'].values())).astype(np.float32))

    def _balance_strip(self, st, names, binned, offs, rpar, B, H, W, out_dir):
        """scope='strip' with balance: every binned range of the call is balanced towards ONE reference, the lower median key of all of
        them (one group, one device-to-host read), in batches of B tiles, before the strip's window is fitted on the balanced values."""
        window, count = ops.tile_intensity_window(binned, offs, rpar, H, W, percentiles=(50.0, 50.0), group=[0] * len(rpar))
        reference = [int(v) for v in torch.cat([window[:, :1].to(torch.int64), count[:, None]], dim=1).cpu().numpy()[0]]
        bal = {}
        for i in range(0, len(rpar), B):
            j = min(i + B, len(rpar))
            self._balance_intensity(st, names[i:j], binned, offs[i:j + 1], rpar[i:j], H, W, out_dir, bal, reference)

    def _stretch_intensity(self, st, names, points, offs, rpar, H, W, out_dir, used, strip=None, bal=None):
        """One batch of tiles through a las_io.IntensityStretch: -> (rpar, inten_scale) to rasterise with.  scope='tile': the two
        percentiles of every tile come from the point ranges the rasteriser will see (ops.tile_intensity_window; one device-to-host read
        of window and count per batch); scope='strip': `strip` is the window found once for the whole call.  Every tile's inten_lo /
        inten_hi are replaced in a copy of its LmRasterParams; the scale travels beside them (0: the derived 255 / inten_hi).  `used`
        collects {tile name: [inten_lo, inten_hi, scale or None, count]} over the call and is written to <out_dir>/params/intensity.json."""
        from . import las_io
        from ._lib import LmRasterParams
        if strip is None:
            if st.balance:                                                  # (scope='strip': balanced before the strip's window was fitted)
                self._balance_intensity(st, names, points, offs, rpar, H, W, out_dir, bal)
            window, count = ops.tile_intensity_window(points, offs, rpar, H, W, percentiles=st.percentiles)
            both = torch.cat([window.to(torch.int64), count[:, None]], dim=1).cpu().numpy()      # the one read-back
            wins = [(*las_io.intensity_window(r[0], r[1], r[2], st), int(r[2])) for r in both]
        else:
            wins = [strip] * len(rpar)
        rpar = [LmRasterParams.from_buffer_copy(r) for r in rpar]
        scales = []
        for name, r, (lo, hi, scale, n) in zip(names, rpar, wins):
            r.inten_lo, r.inten_hi = lo, hi
            scales.append(0.0 if scale is None else scale)
            used[name] = [lo, hi, scale, n]
        with open(os.path.join(self._params_dir(out_dir), 'intensity.json'), 'w') as f:
            json.dump(used, f, indent=1)
        return rpar, scales

    def _raster_stretched(self, raster_batch, st, names, plist, points, offs, rpar, H, W, out_dir, used, strip=None, bal=None):
        """One batch into the chain of _las_chain: as it is without an IntensityStretch (no new code runs), else with every tile's fitted
        window in its LmRasterParams and its scale beside them (the one call site of both LAS routes)."""
        if st is None:
            return raster_batch(names, plist, points, offs, rpar)
        rpar, scales = self._stretch_intensity(st, names, points, offs, rpar, H, W, out_dir, used, strip, bal)
        return raster_batch(names, plist, points, offs, rpar, scales)

    def infer_las_to_map(self, las_and_params, work_dirs=None, path_ckpt=None, batch_size=None, merge=True, select=None, ground=None,
                         intensity=None, elevation=None, density=None, label=None, survey=None, colour=None, residue=None, cross=None,
                         threshold=None):
        """LAS tiles -> map-level 3-D lane lines, every stage of the reference's offline chain on this stack:

          LAS file + tile parameter file (utils/io_utils.py:125-150)
            -> points in HBM (las_io.read_las_raw, shifted by las_read_offset)          [laspy read_las in the reference]
            -> BEV tile on the GPU (lm_bev_raster_batch)                                [external Las2BEV tool]
            -> polylines (TilePipeline) -> <name>.json                                  [Runner :690-867]
            -> LAS-frame polylines (coor_img2pc, elevation from the tile) -> pc/<name>.json / .txt   [coor_img2pc.py]
            -> merged + 0.6 m down-sampled lines -> merged.txt / merged_downsample.txt  [merge_lines.py __main__]

        las_and_params: list of (las_path, param_path) in tile order.  Returns (per-tile dict name -> 3-D lines, merged list).
        select: a las_io.PointFilter applied to every file (default: cfg['las_select'], a dict of its arguments): only the records
        that pass it reach the rasteriser; its z_range is in the frame shifted by las_read_offset.
        ground: a las_io.GroundFilter (default: cfg['las_ground'], a dict of its arguments; absent: nothing changes): per batch the
        ground model of every tile is computed on the GPU from the points `select` left; every tile gets an elevation datum under its
        own ground and / or only the points in a range of heights above the ground are rasterised.  The parameters actually used are
        written to <work_dirs>/params/<name>.txt.
        intensity: a las_io.IntensityStretch (default: cfg['las_intensity'], a dict of its arguments; absent: nothing changes): per batch,
        after `select` and `ground`, every tile's intensity window is fitted to two percentiles of the intensities it keeps
        (ops.tile_intensity_window) and stretched (lm_bev_raster_batch_scaled); what was used is written to
        <work_dirs>/params/intensity.json as {tile name: [inten_lo, inten_hi, scale or null, count]}.  scope='strip' is refused here: the
        tiles arrive file by file.  With intensity.balance the batch's points are first balanced in place per ground cell
        (ops.tile_intensity_cells, las_io.balance_gains, ops.tile_intensity_apply: two more device-to-host reads per batch) and the window
        is fitted on the balanced values; what was used is written to <work_dirs>/params/balance.json as {tile name: [reference, known
        cells, cells, smallest gain, largest gain]} and to balance_gains.npy ([tiles, Gy, Gx] float32).  `elevation` reads heights only
        and is not affected.
        elevation: a las_io.ElevationDrape (default: cfg['las_elevation'], a dict of its arguments; absent: nothing changes): after the
        network, the height of every lane vertex is read off the points the rasteriser saw (ops.drape_vertices, one call and one
        device-to-host read per batch: the lower median of the per-pixel minimum heights around the vertex pixel) instead of the tile's
        8-bit elevation channel; a vertex with fewer than min_pixels filled pixels keeps the channel's value.  The 2-D JSON files do not
        change.  What was used is written to <work_dirs>/params/elevation.json as {tile name: [vertices, draped, fallen back]}.
        density: a las_io.GapFill (default: cfg['las_density'], a dict of its arguments; absent: nothing changes): for a scanner that
        delivers fewer returns than pixels.  Between the rasteriser and the network every empty pixel of a tile takes the bytes of the
        nearest return's pixel within the tile's fill radius (ops.tile_gap_fill; ties to the brightest, then highest).  radius_px='auto'
        picks the radius per tile from the tile's gap histogram (ops.tile_gap_hist, one device-to-host read per batch;
        las_io.gap_radius).  The network and the back-projection both get the filled tile; `elevation` reads the points and is not
        affected.  What was used is written to <work_dirs>/params/density.json as {tile name: [radius, hist[0], ..., hist[Rmax + 1]]}.
        label: a las_io.MarkingLabels (default: cfg['las_label'], a dict of its arguments; absent: nothing changes): after the merge every
        input LAS file is labelled against the lines the call returns (`merged`, or the tiles' lines when nothing was merged): one
        lm_las_label_records call per file, with the file's own las_read_offset and `select` - a record `select` dropped is never
        relabelled.  The file comes back as <work_dirs>/labelled/<basename of the input> with the classification (and, with line_ids, the
        point source ID) of the labelled records patched and every other byte as it was; what was done is written to
        <work_dirs>/params/labels.json as {file: [records, labelled, [per-line counts]]}.  A file listed several times is labelled once
        (with the read offset of its first listing); two different files with one basename are refused with a ValueError before anything
        runs.  The return value does not change.
        survey: a las_io.MarkingSurvey (default: cfg['las_survey'], a dict of its arguments; absent: nothing changes): last, the lines the
        call returns are profiled from the returns of every input file, each read once with its own las_read_offset and `select` (one
        lm_las_line_profile_records call per file into one profile, one read-back): per station bin along every line the count, summed
        intensity and lateral spread of the returns the labelling rule gives the line.  The raw bins are written to
        <work_dirs>/params/markings.npy ([n_bins, 6] int64), what las_io.marking_summary reads off them - paint runs, dashed or solid,
        width, intensity - to <work_dirs>/params/markings.json as {line number: summary}.  Without survey.min_intensity a bin counts
        returns, not paint.  The return value does not change.
        colour: a las_io.MarkingColour (default: cfg['las_colour'], a dict of its arguments; absent: nothing changes), with `survey`
        only: the survey's pass over the records (then one lm_las_line_colour_records call per file, still one read-back) also counts,
        per station bin, the returns that carry a colour, sums their R, G, B and counts those that vote yellow.  The table is written to
        <work_dirs>/params/marking_colours.npy ([n_bins, 6] int64), markings.npy keeps its bytes, and every line of markings.json also
        gets the keys of las_io.marking_colours: coloured, yellow, black, rgb, colour ('white', 'yellow' or 'unknown') and run_colours.
        Refused with a ValueError before anything runs: colour without survey; an input file of a point format without R, G, B (0, 1,
        4, 6, 9).  The return value does not change.
        cross: a las_io.CrossSection (default: cfg['las_cross'], a dict of its arguments; absent: nothing changes, file for file and call
        for call): after `survey` / `colour` and before `residue`, the lines the call returns get a cross-section table from every input
        file, each read once with its own las_read_offset and `select` (one lm_las_line_cross_records call per file into one table, one
        read-back): per station bin along every line a row of lateral cells holding the count, the paint count, the summed intensity
        and the summed height of ALL returns of the band.  The table is written to <work_dirs>/params/cross_sections.npy ([n_bins, nl, 4]
        int64), what las_io.cross_summary reads off it - stripes, double, width, separation, extent, offset, crossfall, the centre per
        station - to cross_sections.json as {line number: summary}, and the lines moved onto their paint (las_io.snap_lines) to
        out_pc_seq_json_dir/merged_snapped.txt and merged_snapped_downsample.txt in the format of merged.txt.  With no lines found the
        files are written empty.  The return value and every other output do not change.
        residue: a las_io.PaintResidue (default: cfg['las_residue'], a dict of its arguments; absent: nothing changes): last of all, the
        paint that none of the lines the call returns explains - stop bars, crossing bars, arrows, hatching, a missed line.  Every input
        file is read once with its `select`; the returns at or above residue.min_intensity that lie within `reach` and `z_tol` of a line
        but farther than `clear` from it are gridded, their connected blobs found and described on the GPU (ops.paint_residue, one
        read-back).  The raw statistics are written to <work_dirs>/params/residue.npy ([K,12] int64), the occupied cells to
        residue_cells.npy ([M,3] int32: cx, cy, blob) and what las_io.residue_summary reads off them - centre, area, length, width, fill,
        heading and shape against the nearest line - to residue.json as {blob number from 1: summary}.  With no lines found the three
        files are written empty.  The grid lives in the frame of the first file's las_read_offset.  The return value does not change.
        threshold: a las_io.PaintThreshold (default: cfg['las_threshold'], a dict of its arguments; absent and no stage says 'auto': nothing
        changes, file for file and call for call; absent and a stage says 'auto': PaintThreshold()): after the merge and before `label`,
        the threshold between asphalt and paint is found in the returns themselves.  Against the lines the call returns, every input
        file is read once with its own las_read_offset and `select` (one lm_las_line_hist_records call per file into one table, one
        read-back): per line and per lateral ring a histogram of the intensities.  The table is written to
        <work_dirs>/params/paint_hist.npy ([L, Z, NB] int64), what las_io.paint_threshold reads off it - threshold, separation, supported,
        the counts and shares, for the strip and per line - to paint_threshold.json as {'strip': ..., 'lines': {line number: ...}}.  Every
        min_intensity='auto' of label, survey and residue and paint_intensity='auto' of cross is then replaced by the strip's threshold.
        A strip whose returns support no threshold is a ValueError that names the separation and the counts, raised after the JSON is
        written and before any stage runs - when a stage asked for 'auto'.  With no lines found both files are written empty.
        Order of the stages: select, (binning,) ground, (balance,) intensity, rasteriser, density, network, elevation, (merge,) threshold, label, survey,
        cross, residue.
        Single rank (the merge is sequential over the sorted tiles)."""
        from . import las_io
        opt, stages = self._las_options(dict(select=select, ground=ground, intensity=intensity, elevation=elevation, density=density,
                                             label=label, survey=survey, colour=colour, residue=residue, cross=cross, threshold=threshold),
                                        [p for p, _ in las_and_params])
        select, ground, intensity, elevation, density = (opt[k] for k in ('select', 'ground', 'intensity', 'elevation', 'density'))
        if intensity is not None and intensity.scope == 'strip':
            raise ValueError("intensity: scope='strip' needs the whole strip in one cloud (infer_las_strip_to_map); infer_las_to_map reads "
                             "its tiles file by file, use scope='tile'")
        used, bal = {}, {}
        if path_ckpt:
            self.load_ckpt(path_ckpt)
        B = int(batch_size or self.cfg.get('batch_size', 8))
        H, W = self.cfg.list_img_size_xy[1], self.cfg.list_img_size_xy[0]
        out_dir = work_dirs or self.cfg.get('work_dirs', './work_dirs')
        raster_batch, close = self._las_chain(work_dirs, merge, elevation, density)
        inputs = []
        for i in range(0, len(las_and_params), B):
            chunk = las_and_params[i:i + B]
            pts, offs, rpar, names, plist = [], [0], [], [], []
            for las_path, param_path in chunk:
                params = io_utils.load_pc_2_img_transform_paras(param_path)
                inputs.append((las_path, params['las_read_offset'], select))
                p, _ = las_io.read_las_raw(las_path, self.device, shift=params['las_read_offset'], select=select)
                pts.append(p)
                offs.append(offs[-1] + p.shape[0])
                rpar.append(io_utils.raster_params_from_file(param_path))
                names.append(os.path.splitext(os.path.basename(las_path))[0][0:11])
                plist.append(params)
            pts = torch.cat(pts)
            if ground is not None:
                plist, pts, offs, rpar = self._follow_ground(ground, names, plist, pts, offs, rpar, H, W, out_dir)
            self._raster_stretched(raster_batch, intensity, names, plist, pts, offs, rpar, H, W, out_dir, used, bal=bal)
        result = close()
        self._after_map(opt['threshold'], stages, opt['colour'], inputs, result, out_dir)
        return result

    def _las_chain(self, work_dirs, merge, elevation=None, density=None):
        """The chain behind infer_las_to_map / infer_las_strip_to_map from the rasteriser on: -> (raster_batch, close).
        raster_batch(names, params, points, offsets, raster_params[, inten_scale]) rasterises one batch of tiles out of `points` and runs it through
        the pipeline, the per-tile JSON and the back-projection; close() drains the pipeline, merges and returns (lines3d, merged).
        elevation: a las_io.ElevationDrape or None.  With one, every batch keeps the (points, offsets, raster_params) the rasteriser saw
        until its futures arrive; the vertices of all its tiles then get their heights in one ops.drape_vertices call.
        density: a las_io.GapFill or None.  With one, a batch is rasterised to u8 only, its gaps are filled on the GPU (one read-back of
        the gap histograms per batch), and the filled u8 tile goes to the pipeline and, copied to the host, to the back-projection."""
        from . import coor_img2pc, las_io, merge_lines as ml
        out_dir = work_dirs or self.cfg.get('work_dirs', './work_dirs')
        pc_dir = os.path.join(out_dir, 'out_pc_seq_json_dir')
        os.makedirs(pc_dir, exist_ok=True)
        pipe = TilePipeline(self.net)
        H, W = self.cfg.list_img_size_xy[1], self.cfg.list_img_size_xy[0]
        queue, lines3d, pc_files, draped, filled = [], {}, [], {}, {}

        def polylines(f, name):
            """One tile's future -> its 2-D JSON on disk and (seqs [L, Vmax, 2], lens), None for a tile the reference skips."""
            lanes, _ = f.result()
            packed = io_utils.pack_lane_vertices(np.asarray(lanes, dtype=np.float64))
            io_utils.save_lane_seq_2d(packed, os.path.join(out_dir, name + '.json'), with_pervertex_semantics=True)
            recs = io_utils.lane_records(packed)
            if len(recs) < 2:                           # load_lane_seq yields nothing for < 2 lines: the reference skips the tile
                return None
            lens = [r['seq_len'] for r in recs]
            seqs = np.zeros((len(recs), max(lens), 2))
            for i, r in enumerate(recs):
                seqs[i, :lens[i]] = np.asarray(r['seq'])[:, 0:2]
            return seqs, lens

        def write_3d(name, pc, lens):
            lines = [{'seq': pc[i, :lens[i], :], 'seq_len': lens[i], 'init_vertex': pc[i, 0, :], 'end_vertex': pc[i, lens[i] - 1, :]}
                     for i in range(len(lens))]
            io_utils.save_seqs_json(lines, os.path.join(pc_dir, name + '.json'))
            io_utils.save_seqs_txt(lines, os.path.join(pc_dir, name + '.txt'))
            pc_files.append(os.path.join(pc_dir, name + '.json'))
            lines3d[name] = [l['seq'] for l in lines]

        def finish(futs):
            if elevation is not None:
                return finish_draped(futs)
            for f in futs:
                name, params, u8 = queue.pop(0)
                got = polylines(f, name)
                if got is not None:
                    write_3d(name, coor_img2pc.transform_coordinate_from_img_2_pc(params, got[0], got[1], u8), got[1])

        def finish_draped(futs):
            """The futures of one batch together: 2-D JSON, then one drape call over the vertices of all its tiles and one read-back,
            then the back-projection of every tile with its vertex heights."""
            if not futs:
                return
            entries = [queue.pop(0) for _ in futs]
            kept = entries[0][3]
            assert all(e[3] is kept for e in entries) and len(entries) == len(kept['rpar'])
            tiles = [polylines(f, e[0]) for f, e in zip(futs, entries)]
            vert, voffs = [], [0]
            for got in tiles:
                if got is not None:
                    seqs, lens = got
                    vert += [(int(seqs[i, v, 0]), int(seqs[i, v, 1])) for i in range(len(lens)) for v in range(lens[i])]
                voffs.append(len(vert))
            if vert:
                z, npix = ops.drape_vertices(kept['points'], kept['offs'], kept['rpar'], np.asarray(vert, dtype=np.int32), voffs, H, W,
                                             radius_px=elevation.radius_px)
                both = torch.stack([z, npix.to(torch.float32)]).cpu().numpy()              # the one read-back
                z = np.where(both[1] < elevation.min_pixels, np.float32(np.nan), both[0])
            for j, (e, got) in enumerate(zip(entries, tiles)):
                name, params, u8 = e[0:3]
                draped[name] = [0, 0, 0]
                if got is None:
                    continue
                seqs, lens = got
                vz = np.full(seqs.shape[0:2], np.nan, dtype=np.float32)
                at = voffs[j]
                for i, n in enumerate(lens):
                    vz[i, :n] = z[at:at + n]
                    at += n
                n_draped = int(np.isfinite(vz).sum())
                draped[name] = [voffs[j + 1] - voffs[j], n_draped, voffs[j + 1] - voffs[j] - n_draped]
                write_3d(name, coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs, lens, u8, vertex_z=vz, fit=elevation.fit), lens)
            with open(os.path.join(self._params_dir(out_dir), 'elevation.json'), 'w') as f:
                json.dump(draped, f, indent=1)

        def fill_gaps(names, points, offs, rpar, inten_scale):
            """One batch through `density`: the u8 tile alone (the stem takes it directly), its gap histograms (the one read-back), every
            tile's radius, the filled u8 tile.  `filled` collects {tile name: [radius, hist...]} over the call -> params/density.json."""
            kw = {} if inten_scale is None else {'inten_scale': inten_scale}
            u8 = ops.bev_raster_batch(points, offs, rpar, H, W, u8_only=True, **kw)
            hist = ops.tile_gap_hist(u8, density.max_radius_px).cpu().numpy()
            radii = [las_io.gap_radius(row, density) for row in hist]
            for name, r, row in zip(names, radii, hist):
                filled[name] = [int(r)] + [int(v) for v in row]
            with open(os.path.join(self._params_dir(out_dir), 'density.json'), 'w') as f:
                json.dump(filled, f, indent=1)
            return ops.tile_gap_fill(u8, radii)

        def raster_batch(names, params, points, offs, rpar, inten_scale=None):
            kept = None if elevation is None else {'points': points, 'offs': [int(o) for o in offs], 'rpar': list(rpar)}
            for name, prm in zip(names, params):
                queue.append([name, prm, None] if kept is None else [name, prm, None, kept])
            if density is not None:
                tiles = u8 = fill_gaps(names, points, offs, rpar, inten_scale)
            elif inten_scale is None:
                tiles, u8 = ops.bev_raster_batch(points, offs, rpar, H, W, want_u8=True)
            else:
                tiles, u8 = ops.bev_raster_batch(points, offs, rpar, H, W, want_u8=True, inten_scale=inten_scale)
            u8_host = u8.cpu().numpy()
            for j in range(len(names)):
                queue[len(queue) - len(names) + j][2] = u8_host[j]
            finish(pipe.submit(tiles))

        def close():
            finish(pipe.flush())
            merged = []
            if merge and pc_files:
                merged = ml.merge_lines(pc_files)
                io_utils.save_seqs_list(merged, os.path.join(pc_dir, 'merged.txt'))
                io_utils.save_seqs_list([ml.downsample_seqs(m) for m in merged], os.path.join(pc_dir, 'merged_downsample.txt'))
            return lines3d, merged

        return raster_batch, close

    @staticmethod
    def _strip_layout(param_paths):
        """Parameter files of one strip -> (names, parameter dicts); all must carry the same las_read_offset."""
        names, plist = [], []
        for path in param_paths:
            params = io_utils.load_pc_2_img_transform_paras(path)
            if plist and list(params['las_read_offset']) != list(plist[0]['las_read_offset']):
                raise ValueError(f"{param_paths[0]} and {path} carry different las_read_offset ({plist[0]['las_read_offset']} and "
                                 f"{params['las_read_offset']}): the tiles of one strip share one read offset")
            names.append(os.path.splitext(os.path.basename(path))[0][0:11])
            plist.append(params)
        return names, plist

    @staticmethod
    def _strip_z_range(headers, shift):
        """The z range of the strip binning's lookup grid: the min / max z of the file headers (las_io.parse_header's dicts) minus `shift`,
        widened by a float ulp's worth - it only bounds the grid, never the result.  None where the headers hold no range."""
        z_lo = min([np.inf] + [h['min'][2] - shift[2] for h in headers])
        z_hi = max([-np.inf] + [h['max'][2] - shift[2] for h in headers])
        pad = 1e-3 * max(1.0, abs(z_lo), abs(z_hi))
        return (z_lo - pad, z_hi + pad) if z_lo <= z_hi else None

    def infer_las_strip_to_map(self, las_paths, param_paths, work_dirs=None, path_ckpt=None, batch_size=None, merge=True, select=None,
                               ground=None, intensity=None, elevation=None, density=None, label=None, survey=None, colour=None, residue=None, cross=None,
                               threshold=None, stream=None):
        """A whole strip -> map-level lane lines: the LAS file(s) of the strip are read once, their points are binned into the tiles of
        the layout on the GPU (ops.strip_bin_points: the windows of `param_paths` may overlap and be rotated), and every batch of tiles
        then runs the chain of infer_las_to_map from the rasteriser on.  Same outputs under the same names; a tile is named by the
        first 11 characters of its parameter file's stem.  las_paths: one path or a list; param_paths in tile order.
        select: as for infer_las_to_map, applied to every file of the strip before the binning (the lookup grid of the binning keeps
        the z range of the file headers: a narrower z_range only makes it conservative).
        ground: as for infer_las_to_map, applied per batch of tiles to the binned ranges, i.e. after `select` and the binning.
        intensity: as for infer_las_to_map, after `ground`.  scope='tile': per batch, on the ranges the rasteriser will see (after the
        height selection of `ground`).  scope='strip': one window for every tile, found once over all binned ranges before the batch
        loop - BEFORE `ground`'s height selection, which runs per batch: points it later drops still count for the strip's window.
        With intensity.balance and scope='strip' all binned ranges are balanced, in batches of tiles, towards the median of the whole
        call before that window is fitted (so before `ground` as well); with scope='tile' per batch, after `ground`.
        elevation: as for infer_las_to_map, after the network, on the ranges the rasteriser saw (after `ground` and `intensity`).
        density: as for infer_las_to_map, per batch between the rasteriser and the network.
        label: as for infer_las_to_map, after the merge: every file of `las_paths` is labelled with the layout's las_read_offset and `select`.
        survey: as for infer_las_to_map, last: every file of `las_paths` is surveyed with the layout's las_read_offset and `select`.
        colour: as for infer_las_to_map, in the survey's pass over the files of `las_paths`.
        cross: as for infer_las_to_map, after the survey: every file of `las_paths` is read with the layout's las_read_offset and `select`.
        residue: as for infer_las_to_map, last of all: every file of `las_paths` is read with the layout's las_read_offset and `select`.
        threshold: as for infer_las_to_map, after the merge and before `label`: every file of `las_paths` is read with the layout's
        las_read_offset and `select`.
        stream: a las_io.StripStream (default: cfg['las_stream'], a dict of its arguments; absent: nothing changes, file for file and
        call for call): the strip is never held as one cloud.  Pass A reads every file in chunks of stream.chunk_records records,
        decodes each into one reused scratch cloud (`select` per chunk) and counts it into the tiles (ops.StripBinner); the counts are
        read once.  The tiles are cut into groups (las_io.tile_groups: layout order, cuts at multiples of the batch size, 16 x the
        group's points within stream.binned_budget); pass B reads the files once more per group and scatters them into the group's
        tiles, and the batch loop runs on the group's (binned, offsets) as it does on the whole strip's: the same bits, so every output
        is the same.  The stages after the merge read the files in the same chunks.  What was done goes to
        <out_dir>/params/stream.json.  intensity scope='strip' needs every binned range at once: with a binned_budget and more tiles
        than one batch - more than one group is then possible - it is refused before anything is read."""
        from . import las_io
        if isinstance(las_paths, (str, os.PathLike)):
            las_paths = [las_paths]
        names, plist = self._strip_layout(list(param_paths))
        opt, stages = self._las_options(dict(select=select, ground=ground, intensity=intensity, elevation=elevation, density=density,
                                             label=label, survey=survey, colour=colour, residue=residue, cross=cross, threshold=threshold,
                                             stream=stream), las_paths)
        select, ground, intensity, elevation, density, stream = (opt[k] for k in ('select', 'ground', 'intensity', 'elevation', 'density',
                                                                                  'stream'))
        used, bal = {}, {}
        B = int(batch_size or self.cfg.get('batch_size', 8))
        if stream is not None and stream.binned_budget is not None and intensity is not None and intensity.scope == 'strip' and len(plist) > B:
            raise ValueError(f"intensity: scope='strip' fits one window to every binned range of the strip at once; with stream.binned_budget="
                             f'{stream.binned_budget} the {len(plist)} tiles (batches of {B}) may be cut into several groups, each binned on '
                             f"its own.  Pass binned_budget=None, or use scope='tile'")
        if path_ckpt:
            self.load_ckpt(path_ckpt)
        H, W = self.cfg.list_img_size_xy[1], self.cfg.list_img_size_xy[0]
        out_dir = work_dirs or self.cfg.get('work_dirs', './work_dirs')
        raster_batch, close = self._las_chain(work_dirs, merge, elevation, density)

        def batches(binned, offs, t0, t1, strip=None):
            """The batch loop over the tiles t0 .. t1 - 1, whose point ranges are offs (t1 - t0 + 1 entries) of binned."""
            for i in range(t0, t1, B):
                j = min(i + B, t1)
                batch = (plist[i:j], binned, offs[i - t0:j - t0 + 1], rpar[i:j])
                if ground is not None:
                    batch = self._follow_ground(ground, names[i:j], *batch, H, W, out_dir)
                self._raster_stretched(raster_batch, intensity, names[i:j], *batch, H, W, out_dir, used, strip, bal)

        if plist and stream is not None:
            rpar = [io_utils.raster_params_from_dict(p) for p in plist]
            self._stream_strip(stream, las_paths, names, plist, rpar, select, intensity, B, H, W, out_dir, batches)
        elif plist:
            shift = plist[0]['las_read_offset']
            clouds, headers = [], []
            for path in las_paths:
                p, h = las_io.read_las_raw(path, self.device, shift=shift, select=select)
                clouds.append(p)
                headers.append(h)
            cloud = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
            rpar = [io_utils.raster_params_from_dict(p) for p in plist]
            binned, offs = ops.strip_bin_points(cloud, rpar, H, W, z_range=self._strip_z_range(headers, shift))
            del cloud, clouds
            strip = None
            if intensity is not None and intensity.scope == 'strip':
                if intensity.balance:
                    self._balance_strip(intensity, names, binned, offs, rpar, B, H, W, out_dir)
                strip = self._strip_intensity(intensity, binned, offs, rpar, H, W)
            batches(binned, offs, 0, len(plist), strip)
        result = close()
        if plist:
            self._after_map(opt['threshold'], stages, opt['colour'], [(path, plist[0]['las_read_offset'], select) for path in las_paths], result,
                            out_dir, None if stream is None else stream.chunk_records)
        return result

    def _stream_strip(self, stream, las_paths, names, plist, rpar, select, intensity, B, H, W, out_dir, batches):
        """The chunked route of infer_las_strip_to_map up to the batch loop (`batches`, which it calls once per group of tiles): pass A
        counts every chunk of every file, pass B scatters them once per group.  No file and no cloud is held whole; the device holds
        one chunk's records, one scratch cloud and the binned points of one group."""
        from . import las_io
        shift = plist[0]['las_read_offset']
        files = [las_io.LasChunks(path, stream.chunk_records, self.device) for path in las_paths]      # (the headers only)
        for ch in files if select is not None else ():
            select.for_format(ch.header['point_format'])                     # refused before anything is uploaded
        binner = ops.StripBinner(rpar, H, W, self._strip_z_range([ch.header for ch in files], shift), self.device)
        kept = [0] * len(files)

        def each_cloud(fn, count=False):
            """fn(points) for every chunk of every file, decoded into one scratch cloud that lives as long as the pass."""
            scratch = torch.empty((min(stream.chunk_records, max([ch.header['n_points'] for ch in files] + [1])), 4), device=self.device,
                                  dtype=torch.float32)
            for k, ch in enumerate(files):
                for pts in las_io.decode_chunks(ch, shift, select, scratch):
                    if count:
                        kept[k] += int(pts.shape[0])
                    fn(pts)

        each_cloud(binner.count, count=True)
        counts = binner.counts()                                             # the one read-back of pass A
        groups = las_io.tile_groups(counts, B, stream.binned_budget)
        done = []
        for t0, t1 in groups:
            binner.begin((t0, t1))
            each_cloud(binner.scatter)
            binned, offs = binner.finish()
            done.append({'tiles': [t0, t1], 'points': int(offs[-1]), 'binned_bytes': 16 * int(offs[-1])})
            strip = None
            if intensity is not None and intensity.scope == 'strip':         # (one group: refused otherwise before anything was read)
                if intensity.balance:
                    self._balance_strip(intensity, names[t0:t1], binned, offs, rpar[t0:t1], B, H, W, out_dir)
                strip = self._strip_intensity(intensity, binned, offs, rpar[t0:t1], H, W)
            batches(binned, offs, t0, t1, strip)
            del binned
        with open(os.path.join(self._params_dir(out_dir), 'stream.json'), 'w') as f:
            json.dump({'chunk_records': stream.chunk_records, 'binned_budget': stream.binned_budget, 'batch_size': B,
                       'files': [{'file': os.path.basename(ch.path), 'records': int(ch.header['n_points']), 'chunks': len(ch), 'kept': n}
                                 for ch, n in zip(files, kept)],
                       'tile_counts': [int(c) for c in counts], 'groups': done}, f, indent=1)

    def infer_lane_geometry_segmentation_segmentor(self, path_ckpt=None, mode_view=False, write_lane_vertex=False,
                                                   *, tiles=None, batch_size=None, gt_avail=None):
        """Segmentor config (runner.py:945-1036): {image_name: (seg [1152,1152] u8-valued f32, endpoints [k,2])} over cfg.dataset.test
        (or `tiles=`).  With labels (default: when the split is used) the loop's geometry (bi_seg) and semantic skeleton counters are
        summed and its six lines printed; self.metrics holds them."""
        from . import datasets, metric_utils
        if path_ckpt:
            self.load_ckpt(path_ckpt)
        self._view_notice(mode_view)
        ents = self._entries(None, tiles)
        gt_avail = (tiles is None) if gt_avail is None else (bool(gt_avail) and tiles is None)
        B = int(batch_size or self.cfg.get('batch_size', 8))
        dist = torch.distributed
        world = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        lo, hi, _ = shard.shard_range(len(ents), rank, world)
        mine = ents[lo:hi]
        res = {}
        c = np.zeros(8, dtype=np.float64)          # semantic TP / dets / DG / gts, geometry TP / pts / DG / gts
        for i in range(0, len(mine), B):
            chunk = mine[i:i + B]
            out = self.net({'proj': self._load_batch([p for _, p, _ in chunk])})
            for j, (name, _, ent) in enumerate(chunk):
                seg = out['seg'][j].numpy()
                res[name] = (seg, out['endp_pts'][j])
                if gt_avail:
                    mask = datasets.load_eval_gt(ent, self.cfg, merge_connect_lines=False)['mask']
                    c[0:4] += metric_utils.eval_metric_line_segmentor(seg, mask, bi_seg=False, semantics=2, buff=self.cfg.validate_buffer)[3:7]
                    c[4:8] += metric_utils.eval_metric_line_segmentor(seg, mask, bi_seg=True, semantics=1, buff=self.cfg.validate_buffer)[3:7]
        if world > 1:
            # every rank gets every tile's result (the class maps travel as u8 when that is lossless: 1.3 MB per tile) + one 64-byte
            # all-reduce of the counters
            def small(seg):
                u8 = seg.astype(np.uint8)
                return u8 if np.array_equal(u8.astype(seg.dtype), seg) else seg
            parts = [None] * world
            dist.all_gather_object(parts, {k: (small(v[0]), str(v[0].dtype), v[1]) for k, v in res.items()})
            res = {k: (seg.astype(dt), pts) for part in parts for k, (seg, dt, pts) in part.items()}
            res = {name: res[name] for name, _, _ in ents}
            t = torch.from_numpy(c).to(self.device)
            dist.all_reduce(t)
            c = t.cpu().numpy()
        self.counters = c
        if gt_avail:
            geo, sem = _prf(*c[4:8]), _prf(*c[0:4])
            self.metrics = {'coor_conf_prec': geo[0], 'coor_conf_rec': geo[1], 'coor_conf_f1': geo[2],
                            'sem_conf_prec': sem[0], 'sem_conf_rec': sem[1], 'sem_conf_f1': sem[2]}
            if rank == 0:
                for k, v in self.metrics.items():
                    print(f'{k}={v}')
        return res


for _arg, _row in LAS_STAGES.items():
    if _arg != 'threshold':
        setattr(Runner, '_las_' + _arg, functools.partialmethod(Runner._las_option, _arg, *_row))
