"""Detection evaluation on the device: the reference's `Evaluator` / `COCOEvaluator` (lfd/evaluation/base_evaluator.py,
coco_evaluator.py:13-82) over csrc/evaluate.hip instead of pycocotools.

The definition of the numbers is written out in DESIGN.md ("Evaluation"): COCOeval with iouType 'bbox', useCats 1 and
maxDets [100, 300, 1000], restated from knowledge of pycocotools 2.0.x.  pycocotools is not a dependency and was never run
against this code: AGREEMENT WITH PYCOCOTOOLS ITSELF IS NOT VERIFIED.  tests/golden/coco_eval_oracle.py is the same
definition as plain numpy loops; the kernels are tested against it.

`TT100KEvaluator` is the other protocol the reference uses: the TT100K dataset's official accuracy / recall
(TT100K_train/official_eval.py eval_annos, called from TT100K_train/evaluation.py:70-79) over csrc/evaluate_tt100k.hip.  Its
definition is DESIGN.md 9b; tests/golden/ref_tt100k_eval.npz holds what the reference itself computes and the tests compare
with it exactly.

`WIDERFACEEvaluator` is the WIDERFACE models' protocol: the dataset's easy / medium / hard AP over
csrc/evaluate_widerface.hip.  The reference only writes text files for the dataset's Matlab tools
(WIDERFACE_train/evaluation.py SIO_evaluation); the definition, DESIGN.md 9c, restates those tools from knowledge of them and
AGREEMENT WITH THEM IS NOT VERIFIED.  tests/golden/widerface_eval_oracle.py is the same definition as plain numpy loops.
`write_widerface_results` / `read_widerface_results` are the reference's text files, `load_widerface_mat` the dataset's
ground truth (needs scipy).

Importing this module and constructing an evaluator need no GPU (the ground truth is parsed on the host and uploaded when a
device is first needed); update / update_resident / a non-empty evaluate run on the MI355X only.
"""
import ctypes as C
import json
import os

import numpy as np

__all__ = ['Evaluator', 'COCOEvaluator', 'TT100KEvaluator', 'TYPE45', 'tt100k_results', 'WIDERFACEEvaluator',
           'write_widerface_results', 'read_widerface_results', 'load_widerface_mat']

METRIC_ITEMS = ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
MAX_DETS = (100, 300, 1000)
ERR_CAPACITY, ERR_IMAGE, ERR_LABEL = 1, 2, 4      # LFD_EVAL_ERR_*


class Evaluator(object):

    def update(self, results):
        raise NotImplementedError

    def evaluate(self):
        raise NotImplementedError


def coco_params():
    """(iouThrs [10], recThrs [101], areaRng [4, 2]) as float64, computed on the host exactly as pycocotools' Params does."""
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    area_rng = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
    return iou_thrs, rec_thrs, area_rng


def summarize(precision, recall):
    """The 12 `stats` of COCOeval.summarize for maxDets [100, 300, 1000]: stats[0] is taken at maxDets[0] = 100 while the
    other precision entries use maxDets[-1] = 1000 -- pycocotools' behaviour with this list, not a typo."""
    def mean(x):
        x = x[x > -1]
        return float(np.mean(x)) if x.size else -1.0
    M = precision.shape[4]
    ap = lambda a, m, t=None: mean(precision[:, :, :, a, m] if t is None else precision[t, :, :, a, m])   # noqa: E731
    ar = lambda a, m: mean(recall[:, :, a, m])   # noqa: E731
    last = M - 1
    return np.array([ap(0, 0), ap(0, last, 0), ap(0, last, 5), ap(1, last), ap(2, last), ap(3, last),
                     ar(0, 0), ar(0, min(1, last)), ar(0, last), ar(1, last), ar(2, last), ar(3, last)], np.float64)


def format_display(stats):
    """The reference's display string (coco_evaluator.py:57-77); stats None: nothing was detected."""
    s = '\n'
    if stats is None:
        return s + 'No bboxes detected! Evaluation abort!\n'
    for i, metric in enumerate(METRIC_ITEMS):
        s += '{:<10}:{:.5f}\n'.format(metric, stats[i])
    return s


class _DeviceEvaluator(Evaluator):
    """What the three evaluators share: the lazily built device state, the detection store of csrc/eval_store.h (grown on
    demand), the bufs struct, the frames of the two append paths, the status word and the display string.  A subclass names
    its store columns, the device tensors its bufs struct points to and its _lib struct, uploads its ground truth in
    `_upload` and describes the problem in `_desc`."""
    _COLUMNS = dict(det_box=((4,), 'float64'), det_score=((), 'float64'), det_img=((), 'int32'), det_cat=((), 'int32'))
    _STORE = ('det_box', 'det_score', 'det_img', 'det_cat')      # the columns this protocol's store has
    _BUFS = ()                 # further device-state tensors of the bufs struct ('img_mask' among them: the protocol has one)
    _BUFS_STRUCT = None        # the struct's ctypes mirror in _lib
    _ERR_LABEL = None          # what LFD_EVAL_ERR_LABEL means to the caller; None: the protocol never raises it
    _image_key = None          # meta['image_id'] -> key of _img_ord, where the two differ

    def _start(self, device):
        """the accumulation state; with a GPU the ground truth is uploaded once, here"""
        self._device = device
        self._eval_display_str = ''
        self._dev = None           # device state, built on first use
        self._seen = set()         # image ordinals since the last evaluate() (_ordinals)
        self._upper = 0            # upper bound of the detections stored on the device
        self._last = None
        import torch
        if torch.cuda.is_available():
            self._state()

    # ------------------------------------------------------------------ device state
    def _state(self):
        if self._dev is not None:
            return self._dev
        import torch
        from . import _lib
        if not torch.cuda.is_available():
            raise RuntimeError('%s: the evaluation kernels run on the MI355X only; there is no CPU implementation' % type(self).__name__)
        dev = torch.device(self._device) if self._device is not None else torch.device('cuda', torch.cuda.current_device())
        d = type('EvalDeviceState', (), {})()
        d.torch, d.lib, d.dev = torch, _lib, dev
        d.fields = self._STORE + ('state',) + self._BUFS           # what _bufs points the struct to
        self._upload(d, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        d.state = torch.zeros(4, dtype=torch.int32, device=dev)
        if 'img_mask' in self._BUFS:
            d.img_mask = torch.zeros(len(self.image_ids), dtype=torch.int32, device=dev)
        d.cap = 0
        for k in self._STORE:
            setattr(d, k, None)
        self._dev = d
        self._reserve(1 << 16)
        return d

    def _reserve(self, need):
        """grow the detection store to hold `need` entries (device-to-device copies on the current stream, no sync)"""
        d = self._dev
        if need <= d.cap:
            return
        torch = d.torch
        cap = max(int(need), 2 * d.cap)
        for k in self._STORE:
            shape, dtype = self._COLUMNS[k]
            new = torch.empty((cap,) + shape, dtype=getattr(torch, dtype), device=d.dev)
            if d.cap:
                new[:d.cap].copy_(getattr(d, k))
            setattr(d, k, new)
        d.cap = cap

    def _bufs(self, **extra):
        d = self._dev
        b = getattr(d.lib, self._BUFS_STRUCT)()
        for k in d.fields:
            setattr(b, k, getattr(d, k).data_ptr())
        for k, t in extra.items():
            setattr(b, k, t.data_ptr() if t is not None else None)
        return b

    def _ordinals(self, meta_batch):
        """image ordinals of a batch; an unknown id, or one that already arrived since the last evaluate(), is a ValueError"""
        ords = []
        for m in meta_batch:
            key = m['image_id'] if self._image_key is None else self._image_key(m['image_id'])
            if key not in self._img_ord:
                raise ValueError('image id %r is not in the annotations' % (key,))
            o = self._img_ord[key]
            if o in self._seen or o in ords:
                raise ValueError('image id %r arrived twice before evaluate()' % (key,))
            ords.append(o)
        return ords

    # ------------------------------------------------------------------ accumulation
    @staticmethod
    def _split(results):
        if not (isinstance(results, tuple) and len(results) == 2):
            raise TypeError('update info should contain two parts: predict bboxes and meta info.')
        predict, meta_batch = results
        if len(predict) != len(meta_batch):
            raise ValueError('%d prediction lists for %d meta entries' % (len(predict), len(meta_batch)))
        return predict, meta_batch

    def _append_rows(self, name, rows, cols, mark=None):
        """_lib `name`(desc, bufs, rows [len(rows), cols] float64, len(rows)[, mark, len(mark)], stream); mark: a list of image
        ordinals where the entry point takes one"""
        d = self._state()
        torch = d.torch
        self._upper += len(rows)
        self._reserve(self._upper)
        with torch.cuda.device(d.dev):
            rows_t = torch.from_numpy(np.array(rows, np.float64).reshape(len(rows), cols)).to(d.dev) if rows else None
            tail = ()
            if mark is not None:
                mark_t = torch.tensor(mark, dtype=torch.int32).to(d.dev) if mark else None
                tail = (d.lib.ptr(mark_t), len(mark))
            desc, bufs = self._desc(), self._bufs()
            d.lib.check(getattr(d.lib.lib(), name)(C.byref(desc), C.byref(bufs), d.lib.ptr(rows_t), len(rows), *tail, d.lib.stream_ptr()), name)

    def _append_resident(self, name, outputs, meta_batch, tail, dummy_rows=0):
        """The frame of update_resident: _lib `name`(desc, bufs, dets, labels, counts, n, cap, *tail(d, ordinals), stream); an
        image takes at most cap + dummy_rows store entries.  -> the batch's image ordinals"""
        n, cap = int(outputs.dets.size(0)), int(outputs.dets.size(1))
        if len(meta_batch) != n:
            raise ValueError('%d meta entries for a batch of %d' % (len(meta_batch), n))
        ords = self._ordinals(meta_batch)
        d = self._state()
        torch = d.torch
        if outputs.dets.device != d.dev:
            raise RuntimeError('update_resident: the outputs live on %s, the evaluator on %s' % (outputs.dets.device, d.dev))
        self._upper += n * (cap + dummy_rows)
        self._reserve(self._upper)
        with torch.cuda.device(d.dev):
            host = torch.empty(n, dtype=torch.int32, pin_memory=True)
            host.numpy()[:] = ords
            ord_t = host.to(d.dev, non_blocking=True)
            desc, bufs = self._desc(), self._bufs()
            d.lib.check(getattr(d.lib.lib(), name)(C.byref(desc), C.byref(bufs), d.lib.ptr(outputs.dets), d.lib.ptr(outputs.labels),
                                                   d.lib.ptr(outputs.counts), n, cap, *tail(d, d.lib.ptr(ord_t)), d.lib.stream_ptr()), name)
        return ords

    # ------------------------------------------------------------------ evaluation
    def _status_error(self, err):
        """the RuntimeError for the status bits `err` (LFD_EVAL_ERR_*) that an evaluate() found"""
        msgs = [m for bit, m in ((ERR_CAPACITY, 'the detection store overflowed'), (ERR_IMAGE, 'an image ordinal was out of range'),
                                 (ERR_LABEL, self._ERR_LABEL)) if err & bit and m]
        return RuntimeError('%s: ' % type(self).__name__ + '; '.join(msgs) +
                            ' (status bits %d); the accumulated detections were dropped' % err)

    def _clear(self):
        self._seen = set()
        self._upper = 0
        if self._dev is not None:
            self._dev.state.zero_()
            if 'img_mask' in self._BUFS:
                self._dev.img_mask.zero_()

    def get_eval_display_str(self):
        return self._eval_display_str


class COCOEvaluator(_DeviceEvaluator):
    """Drop-in for the reference's COCOEvaluator (config_dict['evaluator']): same constructor arguments, `update`,
    `evaluate`, `get_eval_display_str`; plus `update_resident` for ops.DetectOutputs that never leave the device.

    annotation_path: a COCO instances_*.json; annotations: the same structure as a dict (one of the two).
    all_images=False keeps the reference's quirk: an image is evaluated only if it produced at least one detection
    (coco_evaluator.py:47-53), so an image with ground truth and no detection does not count against recall;
    all_images=True evaluates every image passed to update / update_resident."""

    def __init__(self, annotation_path=None, label_indexes_to_category_ids=None, annotations=None, device=None, all_images=False):
        if (annotation_path is None) == (annotations is None):
            raise ValueError('give exactly one of annotation_path and annotations')
        if not isinstance(label_indexes_to_category_ids, dict):
            raise TypeError('label index to category id must be a dict!!!')
        if annotation_path is not None:
            if not os.path.isfile(annotation_path):
                raise FileNotFoundError('annotation file does not exist!!! (%s)' % annotation_path)
            with open(annotation_path) as f:
                annotations = json.load(f)
        if not isinstance(annotations, dict) or 'annotations' not in annotations:
            raise ValueError("annotations must be a COCO dict with an 'annotations' list")
        self._label_indexes_to_category_ids = dict(label_indexes_to_category_ids)
        self._all_images = bool(all_images)
        self._parse(annotations)
        self.iou_thrs, self.rec_thrs, self.area_rng = coco_params()
        self.max_dets = MAX_DETS
        self.stats = self.precision = self.recall = None
        self._host_rows = 0        # rows appended through update()
        self._resident_calls = 0
        self._start(device)

    # ------------------------------------------------------------------ ground truth (host)
    def _parse(self, ann):
        anns = ann['annotations']
        image_ids = set(im['id'] for im in ann.get('images', ())) | set(a['image_id'] for a in anns)
        cat_ids = set(c['id'] for c in ann.get('categories', ())) | set(a['category_id'] for a in anns)
        if not image_ids or not cat_ids:
            raise ValueError('the annotations name no image or no category')
        self.image_ids = sorted(image_ids)
        self.category_ids = sorted(cat_ids)
        self._img_ord = {v: i for i, v in enumerate(self.image_ids)}
        self._cat_idx = {v: i for i, v in enumerate(self.category_ids)}
        for lab, cid in self._label_indexes_to_category_ids.items():
            if cid not in self._cat_idx:
                raise ValueError('label %r maps to category id %r, which the annotations do not have' % (lab, cid))
        I, K, G = len(self.image_ids), len(self.category_ids), len(anns)
        pair = np.array([self._img_ord[a['image_id']] * K + self._cat_idx[a['category_id']] for a in anns], np.int64).reshape(G)
        order = np.argsort(pair, kind='stable')
        box = np.array([a['bbox'] for a in anns], np.float64).reshape(G, 4)
        area = np.array([a['area'] if 'area' in a else a['bbox'][2] * a['bbox'][3] for a in anns], np.float64).reshape(G)
        crowd = np.array([int(a.get('iscrowd', 0)) for a in anns], np.int32).reshape(G)
        self.gt_pair = pair[order]
        self.gt_box, self.gt_area, self.gt_crowd = box[order], area[order], crowd[order]
        self.gt_pair_start = np.searchsorted(self.gt_pair, np.arange(I * K + 1), side='left').astype(np.int32)
        lmax = max([int(l) for l in self._label_indexes_to_category_ids] + [0])
        self._label_map = np.full(lmax + 1, -1, np.int32)
        for lab, cid in self._label_indexes_to_category_ids.items():
            if int(lab) >= 0:
                self._label_map[int(lab)] = self._cat_idx[cid]

    # ------------------------------------------------------------------ device state
    _BUFS = ('img_mask', 'gt_box', 'gt_area', 'gt_crowd', 'gt_pair_start', 'iou_thrs', 'area_rng', 'rec_thrs')
    _BUFS_STRUCT = 'EvalBufs'
    _ERR_LABEL = 'a detection carried a label that label_indexes_to_category_ids does not map'

    def _upload(self, d, up):
        G = len(self.gt_area)
        d.gt_box = up(self.gt_box if G else np.zeros((1, 4)))
        d.gt_area = up(self.gt_area if G else np.zeros(1))
        d.gt_crowd = up(self.gt_crowd if G else np.zeros(1, np.int32))
        d.gt_pair_start = up(self.gt_pair_start)
        d.iou_thrs, d.rec_thrs, d.area_rng = up(self.iou_thrs), up(self.rec_thrs), up(self.area_rng)
        d.label_map = up(self._label_map)

    def _desc(self):
        d = self._dev
        desc = d.lib.EvalDesc()
        desc.num_images, desc.num_categories = len(self.image_ids), len(self.category_ids)
        desc.num_gt, desc.det_capacity = len(self.gt_area), d.cap
        desc.num_iou_thrs, desc.num_area_rngs = len(self.iou_thrs), len(self.area_rng)
        desc.num_rec_thrs, desc.num_max_dets = len(self.rec_thrs), len(self.max_dets)
        for i, m in enumerate(self.max_dets):
            desc.max_dets[i] = int(m)
        return desc

    def _ordinals(self, meta_batch):
        try:
            return [self._img_ord[m['image_id']] for m in meta_batch]
        except KeyError as e:
            raise ValueError('image id %s is not in the annotations' % e)

    # ------------------------------------------------------------------ accumulation
    def update(self, results):
        """results: tuple(predict_bboxes, meta_batch); predict_bboxes[i] is a list of [label, score, x, y, w, h] rows for
        image meta_batch[i]['image_id'] (what LFD.get_results returns)."""
        predict_bboxes, meta_batch = self._split(results)
        ords = self._ordinals(meta_batch)
        rows = []
        for o, boxes in zip(ords, predict_bboxes):
            for r in boxes:
                cid = self._label_indexes_to_category_ids[r[0]]      # KeyError for an unknown label, as the reference
                rows.append((o, self._cat_idx[cid], r[1], r[2], r[3], r[4], r[5]))
        mark = ords if self._all_images else []
        if not rows and not mark:
            return
        self._append_rows('lfd_eval_append_rows_f64', rows, 7, mark)
        self._host_rows += len(rows)

    def update_resident(self, outputs, meta_batch):
        """Appends the kept boxes of an ops.DetectOutputs (LFD.detect / detect_resident) on the device: no .item(),
        .tolist(), .cpu() or synchronisation; the number of kept boxes is read from outputs.counts by the kernel.  The only
        host -> device traffic is the batch's image ordinals (pinned, asynchronous)."""
        self._append_resident('lfd_eval_append_dets_f32', outputs, meta_batch,
                              lambda d, ords: (d.lib.ptr(d.label_map), int(d.label_map.numel()), ords, int(self._all_images)))
        self._resident_calls += 1

    # ------------------------------------------------------------------ evaluation
    def _run(self, timing=None):
        """enqueue both stages; returns the device tensors (no synchronisation)"""
        d = self._state()
        torch, lib = d.torch, d.lib
        T, R, K, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.category_ids), len(self.area_rng), len(self.max_dets)
        with torch.cuda.device(d.dev):
            i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=d.dev)   # noqa: E731
            i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=d.dev)   # noqa: E731
            out = dict(order=i32(d.cap), sort_key=i64(d.cap), sorted_cat=i32(d.cap), sorted_rank=i32(d.cap),
                       match_bits=i64(d.cap), ignore_bits=i64(d.cap), npig=i32(K, A), cat_start=i32(K + 1),
                       precision=torch.empty((T, R, K, A, M), dtype=torch.float64, device=d.dev),
                       recall=torch.empty((T, K, A, M), dtype=torch.float64, device=d.dev))
            desc, bufs = self._desc(), self._bufs(**out)
            wm = lib.lib().lfd_eval_match_workspace_bytes(C.byref(desc))
            wa = lib.lib().lfd_eval_accumulate_workspace_bytes(C.byref(desc))
            if wm == 0 or wa == 0:
                raise RuntimeError('COCOEvaluator: this problem size is not supported by the evaluation kernels')
            ws_m = torch.empty(wm, dtype=torch.uint8, device=d.dev)
            ws_a = torch.empty(wa, dtype=torch.uint8, device=d.dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timing is not None else None
            if ev:
                ev[0].record()
            lib.check(lib.lib().lfd_eval_match(C.byref(desc), C.byref(bufs), lib.ptr(ws_m), wm, lib.stream_ptr()), 'lfd_eval_match')
            if ev:
                ev[1].record()
            lib.check(lib.lib().lfd_eval_accumulate(C.byref(desc), C.byref(bufs), lib.ptr(ws_a), wa, lib.stream_ptr()),
                      'lfd_eval_accumulate')
            if ev:
                ev[2].record()
                timing.append(ev)
        out['ws'] = (ws_m, ws_a)
        return out

    def evaluate(self, keep_matches=False):
        """Runs both stages on what update / update_resident accumulated, fills `stats` (12 values), `precision`
        [T, R, K, A, M] and `recall` [T, K, A, M] (numpy), builds the display string and clears the accumulated
        detections.  keep_matches=True keeps the per-detection flags of stage 1 for `match_table()`."""
        self.stats = self.precision = self.recall = None
        self._last = None
        if self._host_rows == 0 and self._resident_calls == 0:
            self._eval_display_str = format_display(None)
            self._clear()
            return
        d = self._state()
        torch = d.torch
        out = self._run()
        with torch.cuda.device(d.dev):
            tail = torch.cat([out['precision'].reshape(-1), out['recall'].reshape(-1), d.state.double()]).cpu().numpy()   # the one D2H
        np_, nr = out['precision'].numel(), out['recall'].numel()
        state = tail[np_ + nr:].astype(np.int64)
        err = int(state[1])
        n_det = int(state[0])
        if keep_matches and not err:
            n = int(state[2])
            self._last = dict((k, out[k][:n].cpu().numpy()) for k in ('order', 'sorted_cat', 'sorted_rank', 'match_bits', 'ignore_bits'))
            self._last['npig'] = out['npig'].cpu().numpy()
            self._last['n_det'] = n_det
        self._clear()
        if err:
            raise self._status_error(err)
        if n_det == 0:
            self._eval_display_str = format_display(None)
            return
        self.precision = tail[:np_].reshape(out['precision'].shape)
        self.recall = tail[np_:np_ + nr].reshape(out['recall'].shape)
        self.stats = summarize(self.precision, self.recall)
        self._eval_display_str = format_display(self.stats)

    def match_table(self):
        """After evaluate(keep_matches=True): dict of numpy arrays, one row per detection that took part --
        `index` (insertion index), `category` (index), `rank` (inside its (image, category) pair), `matched` and `ignored`
        [n, T, A] bool; plus `npig` [K, A]."""
        if self._last is None:
            raise RuntimeError('match_table: call evaluate(keep_matches=True) first')
        T, A = len(self.iou_thrs), len(self.area_rng)
        bits = np.arange(T * A, dtype=np.uint64)
        unpack = lambda v: ((v.astype(np.uint64)[:, None] >> bits) & np.uint64(1)).astype(bool).reshape(-1, T, A)   # noqa: E731
        return dict(index=self._last['order'], category=self._last['sorted_cat'], rank=self._last['sorted_rank'],
                    matched=unpack(self._last['match_bits']), ignored=unpack(self._last['ignore_bits']), npig=self._last['npig'])

    def _clear(self):
        self._host_rows = self._resident_calls = 0
        super(COCOEvaluator, self)._clear()


# ====================================================================== TT100K: the dataset's official accuracy / recall
# the 45 categories the reference evaluates (official_eval.type45), in its order
TYPE45 = ['i2', 'i4', 'i5', 'il100', 'il60', 'il80', 'io', 'ip', 'p10', 'p11', 'p12', 'p19', 'p23', 'p26', 'p27', 'p3', 'p5', 'p6',
          'pg', 'ph4', 'ph4.5', 'ph5', 'pl100', 'pl120', 'pl20', 'pl30', 'pl40', 'pl5', 'pl50', 'pl60', 'pl70', 'pl80', 'pm20',
          'pm30', 'pm55', 'pn', 'pne', 'po', 'pr40', 'w13', 'w32', 'w55', 'w57', 'w59', 'wo']
DET_EXCLUDED, DET_RIGHT, DET_WRONG, DET_UNMATCHED = 0, 1, 2, 3      # LFD_TT100K_DET_*
GT_EXCLUDED, GT_MISSED, GT_MATCHED = 0, 1, 2                        # LFD_TT100K_GT_*


def _names_of(label_indexes_to_category_names):
    """dict or list (dataset.meta_info['label_indexes_to_category_names']) -> dict label -> name"""
    m = label_indexes_to_category_names
    if isinstance(m, dict):
        return dict((int(k), str(v)) for k, v in m.items())
    if isinstance(m, (list, tuple)):
        return dict((i, str(v)) for i, v in enumerate(m))
    raise TypeError('label index to category name must be a dict or a list!!!')


def tt100k_results(predict_results, meta_batch, label_indexes_to_category_names):
    """The results dictionary of TT100K_train/evaluation.py:42-57 ({'imgs': {id: {'id', 'objects': [{'bbox', 'category',
    'score'}]}}}) from LFD.get_results rows [label, score, x, y, w, h]: score * 100, xmax = w + x, ymax = h + y.  json.dump it
    to get the file the dataset's official tool reads."""
    names = _names_of(label_indexes_to_category_names)
    if len(predict_results) != len(meta_batch):
        raise ValueError('%d prediction lists for %d meta entries' % (len(predict_results), len(meta_batch)))
    out = dict(imgs=dict())
    for meta, results in zip(meta_batch, predict_results):
        image_id = str(meta['image_id'])
        temp = dict(id=image_id, objects=list())
        for result in results:
            temp['objects'].append(dict(bbox={'xmin': result[2], 'ymin': result[3], 'xmax': result[4] + result[2],
                                              'ymax': result[5] + result[3]},
                                        category=names[result[0]], score=result[1] * 100))
        out['imgs'][image_id] = temp
    return out


def _ratio(right, n):
    return 1 if n == 0 else right * 1.0 / n      # the reference's expression: the int 1 when nothing was counted


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v]


class TT100KEvaluator(_DeviceEvaluator):
    """The TT100K protocol as config_dict['evaluator']: `update`, `update_resident`, `evaluate`, `get_eval_display_str` as
    COCOEvaluator.  The defaults reproduce the reference's call (iou 0.5, minscore 90, sizes [0, 400), the 45 types,
    check_type and match_same on).

    annotation_path: the dataset's annotations.json; annotations: the same structure as a dict (one of the two):
    {'imgs': {id: {'objects': [{'bbox': {'xmin', 'ymin', 'xmax', 'ymax'}, 'category': name}]}}}.
    iou, minscore: a value or a sequence; size_ranges: a sequence of (minboxsize, maxboxsize).  One evaluate() computes every
    combination; the results are indexed [iou, minscore, size range].  types=None: no category filter.
    Every image passed to update / update_resident is evaluated, with or without detections."""

    def __init__(self, annotation_path=None, annotations=None, label_indexes_to_category_names=None, types=TYPE45, iou=0.5,
                 minscore=90, size_ranges=((0, 400),), check_type=True, match_same=True, device=None):
        if (annotation_path is None) == (annotations is None):
            raise ValueError('give exactly one of annotation_path and annotations')
        if annotation_path is not None:
            if not os.path.isfile(annotation_path):
                raise FileNotFoundError('annotation file does not exist!!! (%s)' % annotation_path)
            with open(annotation_path) as f:
                annotations = json.load(f)
        if not isinstance(annotations, dict) or not isinstance(annotations.get('imgs'), dict) or not annotations['imgs']:
            raise ValueError("annotations must be a TT100K dict with a non-empty 'imgs' dict")
        self._names = _names_of(label_indexes_to_category_names)
        self.types = None if types is None else [str(t) for t in types]
        self.ious, self.minscores = _as_list(iou), _as_list(minscore)
        self.size_ranges = [tuple(r) for r in size_ranges]
        if not self.ious or not self.minscores or not self.size_ranges or any(len(r) != 2 for r in self.size_ranges):
            raise ValueError('iou, minscore and size_ranges need at least one entry each; a size range is (min, max)')
        self.check_type, self.match_same = bool(check_type), bool(match_same)
        self._parse(annotations)
        self.right = self.num_detections = self.num_ground_truth = self.accuracy = self.recall = None
        self.right_per_category = self.num_detections_per_category = self.num_ground_truth_per_category = None
        self._start(device)

    # ------------------------------------------------------------------ ground truth (host)
    def _parse(self, ann):
        self.image_ids = [str(k) for k in ann['imgs']]
        self._img_ord = dict((k, i) for i, k in enumerate(self.image_ids))
        if len(self._img_ord) != len(self.image_ids):
            raise ValueError('two image ids of the annotations are the same string')
        cats, box, cat, start = dict(), [], [], [0]
        idx = lambda name: cats.setdefault(str(name), len(cats))   # noqa: E731
        for name in self._names.values():
            idx(name)
        for t in self.types or ():
            idx(t)
        for k in ann['imgs']:
            for obj in ann['imgs'][k].get('objects', ()):
                b = obj['bbox']
                box.append([b['xmin'], b['ymin'], b['xmax'], b['ymax']])
                cat.append(idx(obj['category']))
            start.append(len(cat))
        self.category_names = list(cats)
        self._cat_idx = cats
        self.gt_box = np.array(box, np.float64).reshape(len(cat), 4)
        self.gt_cat = np.array(cat, np.int32).reshape(len(cat))
        self.gt_start = np.array(start, np.int32)
        K = len(cats)
        self._in_types = np.ones(K, np.int32)
        if self.types is not None:
            self._in_types[:] = 0
            self._in_types[[cats[t] for t in self.types]] = 1
        lmax = max([l for l in self._names] + [0])
        self._label_map = np.full(lmax + 1, -1, np.int32)
        for lab, name in self._names.items():
            if lab >= 0:
                self._label_map[lab] = cats[name]

    # ------------------------------------------------------------------ device state
    _BUFS = ('img_mask', 'gt_box', 'gt_cat', 'gt_start', 'cat_in_types', 'ious', 'minscores', 'size_ranges')
    _BUFS_STRUCT = 'TT100KEvalBufs'
    _ERR_LABEL = 'a detection carried a label that label_indexes_to_category_names does not name'
    _image_key = staticmethod(str)

    def _upload(self, d, up):
        G = len(self.gt_cat)
        d.gt_box = up(self.gt_box if G else np.zeros((1, 4)))
        d.gt_cat = up(self.gt_cat if G else np.zeros(1, np.int32))
        d.gt_start = up(self.gt_start)
        d.cat_in_types = up(self._in_types)
        d.ious = up(np.array([float(v) for v in self.ious], np.float64))
        d.minscores = up(np.array([float(v) for v in self.minscores], np.float64))
        d.size_ranges = up(np.array([[float(lo), float(hi)] for lo, hi in self.size_ranges], np.float64))
        d.label_map = up(self._label_map)

    def _desc(self):
        d = self._dev
        desc = d.lib.TT100KEvalDesc()
        desc.num_images, desc.num_categories = len(self.image_ids), len(self.category_names)
        desc.num_gt, desc.det_capacity = len(self.gt_cat), d.cap
        desc.num_ious, desc.num_minscores, desc.num_size_ranges = len(self.ious), len(self.minscores), len(self.size_ranges)
        desc.check_type, desc.match_same = int(self.check_type), int(self.match_same)
        return desc

    # ------------------------------------------------------------------ accumulation
    def update(self, results):
        """results: tuple(predict_results, meta_batch); predict_results[i] is a list of [label, score, x, y, w, h] rows for
        image meta_batch[i]['image_id'] (what LFD.get_results / predict_for_single_image return)."""
        predict_results, meta_batch = self._split(results)
        ords = self._ordinals(meta_batch)
        rows = []
        for o, boxes in zip(ords, predict_results):
            for r in boxes:
                if r[0] not in self._names:
                    raise ValueError('label %r has no category name' % (r[0],))
                rows.append((o, self._cat_idx[self._names[r[0]]], r[1], r[2], r[3], r[4], r[5]))
        if not ords:
            return
        self._append_rows('lfd_eval_tt100k_append_rows_f64', rows, 7, ords)
        self._seen.update(ords)

    def update_resident(self, outputs, meta_batch):
        """Appends the kept boxes of an ops.DetectOutputs (LFD.detect / detect_resident) on the device: no .item(),
        .tolist(), .cpu() or synchronisation; the number of kept boxes is read from outputs.counts by the kernel, which also
        does the reference's arithmetic (fp32 w = x2 - x1 + 1, float64 xmax = w + x1, score * 100).  The only host -> device
        traffic is the batch's image ordinals (pinned, asynchronous)."""
        ords = self._append_resident('lfd_eval_tt100k_append_dets_f32', outputs, meta_batch,
                                     lambda d, ords: (d.lib.ptr(d.label_map), int(d.label_map.numel()), ords))
        self._seen.update(ords)

    # ------------------------------------------------------------------ evaluation
    def _run(self, keep_matches=False):
        """enqueue the grouping, the matching and the counting; returns the device tensors (no synchronisation)"""
        d = self._state()
        torch, lib = d.torch, d.lib
        T, M, S, K = len(self.ious), len(self.minscores), len(self.size_ranges), len(self.category_names)
        G, I = max(len(self.gt_cat), 1), len(self.image_ids)
        with torch.cuda.device(d.dev):
            i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=d.dev)   # noqa: E731
            u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=d.dev)   # noqa: E731
            out = dict(det_start=i32(I + 1), det_index=i32(d.cap), det_match=i32(T * M, d.cap), gt_match=i32(T * M, G),
                       totals=torch.empty((T, M, S, 3), dtype=torch.int64, device=d.dev),
                       per_category=torch.empty((T, M, S, K, 3), dtype=torch.int64, device=d.dev) if self.match_same else None,
                       det_code=u8(T, M, S, d.cap) if keep_matches else None, gt_code=u8(T, M, S, G) if keep_matches else None)
            desc, bufs = self._desc(), self._bufs(**out)
            wb = lib.lib().lfd_eval_tt100k_workspace_bytes(C.byref(desc))
            if wb == 0:
                raise RuntimeError('TT100KEvaluator: this problem size is not supported by the evaluation kernels')
            ws = torch.empty(wb, dtype=torch.uint8, device=d.dev)
            lib.check(lib.lib().lfd_eval_tt100k_match(C.byref(desc), C.byref(bufs), lib.ptr(ws), wb, lib.stream_ptr()),
                      'lfd_eval_tt100k_match')
        out['ws'] = ws
        return out

    def evaluate(self, keep_matches=False):
        """Runs the kernels on what update / update_resident accumulated and fills `right`, `num_detections`,
        `num_ground_truth` (int64 [T, M, S]), `accuracy`, `recall` (float64, from the integers with the reference's
        expression) and, with match_same, `right_per_category`, `num_detections_per_category`,
        `num_ground_truth_per_category` ([T, M, S, K], K over `category_names`); builds the display string and clears the
        accumulated detections.  keep_matches=True keeps the per-object outcomes for `match_table()`."""
        T, M, S, K = len(self.ious), len(self.minscores), len(self.size_ranges), len(self.category_names)
        self._last = None
        per = None
        if not self._seen:
            tot = np.zeros((T, M, S, 3), np.int64)
            if self.match_same:
                per = np.zeros((T, M, S, K, 3), np.int64)
            self._clear()
        else:
            d = self._state()
            torch = d.torch
            out = self._run(keep_matches)
            with torch.cuda.device(d.dev):
                parts = [out['totals'].reshape(-1), d.state.long()]
                if self.match_same:
                    parts.append(out['per_category'].reshape(-1))
                flat = torch.cat(parts).cpu().numpy()                    # the one D2H
            nt = T * M * S * 3
            tot = flat[:nt].reshape(T, M, S, 3)
            state = flat[nt:nt + 4]
            if self.match_same:
                per = flat[nt + 4:].reshape(T, M, S, K, 3)
            err = int(state[1])
            if keep_matches and not err:
                n = int(state[2])
                self._last = dict(det_start=out['det_start'].cpu().numpy(), det_index=out['det_index'][:n].cpu().numpy(),
                                  det_gt=out['det_match'][:, :n].cpu().numpy().reshape(T, M, n),
                                  det_code=out['det_code'][..., :n].cpu().numpy(),
                                  gt_code=out['gt_code'][..., :len(self.gt_cat)].cpu().numpy())
            self._clear()
            if err:
                raise self._status_error(err)
        self.right, self.num_detections, self.num_ground_truth = tot[..., 0].copy(), tot[..., 1].copy(), tot[..., 2].copy()
        ratios = lambda n: np.array([float(_ratio(int(r), int(v))) for r, v in zip(self.right.ravel(), n.ravel())],   # noqa: E731
                                    np.float64).reshape(T, M, S)
        self.accuracy, self.recall = ratios(self.num_detections), ratios(self.num_ground_truth)
        if per is not None:
            self.right_per_category, self.num_detections_per_category, self.num_ground_truth_per_category = (
                per[..., 0].copy(), per[..., 1].copy(), per[..., 2].copy())
        else:
            self.right_per_category = self.num_detections_per_category = self.num_ground_truth_per_category = None
        self._eval_display_str = '\n'.join(self.report(t, m, s) for t in range(T) for m in range(M) for s in range(S))

    def report(self, t=0, m=0, s=0):
        """the reference's report line for one combination, character for character (a `types` list with a single name
        prints that name, where the reference raises)"""
        if self.right is None:
            raise RuntimeError('report: call evaluate() first')
        if self.types is None:
            styps = 'all'
        else:
            distinct = list(dict.fromkeys(self.types))
            if len(distinct) == 1:
                styps = distinct[0]
            elif not self.check_type or len(distinct) == 0:
                styps = 'none'
            else:
                styps = '[%s, ...total %s...]' % (distinct[0], len(distinct))
        right = int(self.right[t, m, s])
        return 'iou:%s, size:[%s,%s), types:%s, accuracy:%s, recall:%s' % (
            self.ious[t], self.size_ranges[s][0], self.size_ranges[s][1], styps,
            _ratio(right, int(self.num_detections[t, m, s])), _ratio(right, int(self.num_ground_truth[t, m, s])))

    def match_table(self, t=0, m=0, s=0):
        """After evaluate(keep_matches=True), for one combination: dict of numpy arrays.  Per detection that was stored, in
        image order and insertion order inside an image: `image` (ordinal in `image_ids`), `index` (insertion index into the
        accumulation), `det_code` (DET_EXCLUDED / DET_RIGHT / DET_WRONG / DET_UNMATCHED) and `det_gt` (index of the matched
        ground truth inside its image's annotation list, -1 unmatched, -2 taken out before the matching); `det_start`
        [images + 1]; per ground truth in annotation order `gt_code` (GT_EXCLUDED / GT_MISSED / GT_MATCHED) with `gt_start`.
        The reference's `right` are the DET_RIGHT detections, `wrong` DET_WRONG and DET_UNMATCHED, `miss` GT_MISSED."""
        if self._last is None:
            raise RuntimeError('match_table: call evaluate(keep_matches=True) first')
        L = self._last
        start = L['det_start']
        return dict(image=np.repeat(np.arange(len(start) - 1), np.diff(start)), index=L['det_index'], det_start=start,
                    det_code=L['det_code'][t, m, s], det_gt=L['det_gt'][t, m], gt_code=L['gt_code'][t, m, s], gt_start=self.gt_start)


# ====================================================================== WIDERFACE: easy / medium / hard AP
DIFFICULTIES = ('easy', 'medium', 'hard')
NUM_THRESHOLDS = 1000


def widerface_thresholds(T=NUM_THRESHOLDS):
    """thr[t] = 1 - (t + 1) / T in float64, computed on the host and handed to the kernels as a table"""
    return np.array([1 - (t + 1) / T for t in range(T)], np.float64)


def _annotation_index(annotations):
    index = dict()
    for i, a in enumerate(annotations):
        if a['id'] in index:
            raise ValueError('image id %r appears twice in the annotations' % (a['id'],))
        index[a['id']] = i
    return index


def voc_ap(rec, prec):
    """VOC's VOCap: pad, running maximum of the precision from the right, and the sum of (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    over the i where mrec changes, added in ascending order one after the other (float64)."""
    mrec = np.concatenate([[0.0], np.asarray(rec, np.float64), [1.0]])
    mpre = np.concatenate([[0.0], np.asarray(prec, np.float64), [0.0]])
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = np.float64(0.0)
    for i in np.nonzero(mrec[1:] != mrec[:-1])[0]:
        ap = ap + (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return float(ap)


def widerface_ap(curve, faces):
    """step 6 of DESIGN.md 9c: (precision [3, T], recall [3, T], ap [3]) in float64 from the integer curve [3, T, 2] and faces
    [3].  Where no proposal was counted the precision is 0 (the dataset's tools have NaN there; the recall count is 0 there
    as well, so the AP does not depend on the choice)."""
    curve, faces = np.asarray(curve, np.int64), np.asarray(faces, np.int64)
    prop, rec = curve[..., 0].astype(np.float64), curve[..., 1].astype(np.float64)
    precision = np.zeros_like(rec)
    np.divide(rec, prop, out=precision, where=prop != 0)
    recall = np.zeros_like(rec)
    den = np.broadcast_to(faces.astype(np.float64)[:, None], rec.shape)
    np.divide(rec, den, out=recall, where=den != 0)
    ap = np.array([voc_ap(recall[d], precision[d]) for d in range(curve.shape[0])], np.float64)
    return precision, recall, ap


def _quantise_as_written(r):
    """SIO_evaluation line 41 on one row [label, score, x, y, w, h] -> (score, x, y, w, h) as the text file keeps them"""
    import math
    return (float('%.03f' % min(r[1], 1)), float(math.floor(r[2])), float(math.floor(r[3])), float(math.ceil(r[4])),
            float(math.ceil(r[5])))


def write_widerface_results(predict_results, meta_batch, annotations, results_save_root):
    """The text files that the reference's WIDERFACE_train/evaluation.py SIO_evaluation leaves for the dataset's Matlab
    tools: <results_save_root>/<event>/<stem>.txt holding the stem, the number of rows + 1, the dummy row '0 0 0 0 0.001' and
    one 'x y w h score' row per detection (floor x, floor y, ceil w, ceil h as integers, min(score, 1) with three decimals).
    predict_results[i]: rows [label, score, x, y, w, h] of image meta_batch[i]['image_id']; event and stem come from
    `annotations`."""
    if len(predict_results) != len(meta_batch):
        raise ValueError('%d prediction lists for %d meta entries' % (len(predict_results), len(meta_batch)))
    index = _annotation_index(annotations)
    for meta, rows in zip(meta_batch, predict_results):
        if meta['image_id'] not in index:
            raise ValueError('image id %r is not in the annotations' % (meta['image_id'],))
        a = annotations[index[meta['image_id']]]
        lines = [a['stem'], '%d' % (len(rows) + 1), '0 0 0 0 0.001']
        for r in rows:
            score, x, y, w, h = _quantise_as_written(r)
            lines.append('%d %d %d %d %.3f' % (x, y, w, h, score))
        event_dir = os.path.join(results_save_root, a['event'])
        os.makedirs(event_dir, exist_ok=True)
        with open(os.path.join(event_dir, a['stem'] + '.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


def read_widerface_results(root, annotations):
    """Reads a directory that write_widerface_results (or the reference) wrote: -> (predict_results, meta_batch) for
    WIDERFACEEvaluator.update, rows [0, score, x, y, w, h] with the dummy row included, one entry per annotated image that
    has a file.  Fed to an evaluator with as_written=False they give what as_written=True gives on the original rows."""
    predict_results, meta_batch = [], []
    for a in annotations:
        path = os.path.join(root, a['event'], a['stem'] + '.txt')
        if not os.path.isfile(path):
            continue
        with open(path) as f:
            lines = [l for l in f.read().splitlines() if l.strip()]
        n = int(lines[1])
        rows = []
        for l in lines[2:2 + n]:
            v = l.split()
            rows.append([0, float(v[4]), float(v[0]), float(v[1]), float(v[2]), float(v[3])])
        if len(rows) != n:
            raise ValueError('%s announces %d rows and holds %d' % (path, n, len(rows)))
        predict_results.append(rows)
        meta_batch.append(dict(image_id=a['id']))
    return predict_results, meta_batch


def load_widerface_mat(gt_dir):
    """The dataset's ground truth (wider_face_val.mat and wider_{easy,medium,hard}_val.mat in gt_dir) as the annotation list
    of WIDERFACEEvaluator; an image's id is its file stem.  The keep lists of the .mat files are 1-based and become 0-based
    here.  Needs scipy (ImportError without it); nothing else in the package does."""
    try:
        from scipy.io import loadmat
    except ImportError:
        raise ImportError('load_widerface_mat needs scipy to read the .mat files')
    gt = loadmat(os.path.join(gt_dir, 'wider_face_val.mat'))
    keep = dict((d, loadmat(os.path.join(gt_dir, 'wider_%s_val.mat' % d))['gt_list']) for d in DIFFICULTIES)
    annotations = []
    for e in range(len(gt['event_list'])):
        event = str(np.asarray(gt['event_list'][e][0]).ravel()[0])
        files = gt['file_list'][e][0]
        for i in range(len(files)):
            stem = str(np.asarray(files[i][0]).ravel()[0])
            boxes = np.asarray(gt['face_bbx_list'][e][0][i][0], np.float64).reshape(-1, 4)
            lists = dict((d, (np.asarray(keep[d][e][0][i][0], np.int64).reshape(-1) - 1).tolist()) for d in DIFFICULTIES)
            annotations.append(dict(id=stem, event=event, stem=stem, boxes=boxes, keep=lists))
    return annotations


class WIDERFACEEvaluator(_DeviceEvaluator):
    """The WIDERFACE protocol as config_dict['evaluator']: `update`, `update_resident`, `evaluate`, `get_eval_display_str` as
    the other two evaluators; evaluate() returns {'easy': ap, 'medium': ap, 'hard': ap}.  The definition is DESIGN.md 9c: a
    restatement of the dataset's eval_tools (wider_eval.m, evaluation.m, read_pred.m, norm_score.m, boxoverlap.m) and VOC's
    VOCap from knowledge of them and of the widely used Python port.  AGREEMENT WITH THOSE TOOLS IS NOT VERIFIED.

    annotations: an ordered list of images, each a dict with 'id' (what meta['image_id'] carries), 'event' and 'stem' (used
    by write_widerface_results only), 'boxes' ([G, 4] x, y, w, h) and 'keep' ({'easy' | 'medium' | 'hard': 0-based indices
    into boxes}); load_widerface_mat builds it from the dataset's .mat files.
    as_written=True evaluates what the reference's text files hold instead of the rows themselves: floor x, floor y, ceil w,
    ceil h, min(score, 1) to three decimals, and the dummy row 0 0 0 0 0.001 first in every image passed to update /
    update_resident.  label_index: detections with another label are dropped.
    faces[d] counts the keep lists of EVERY annotated image, passed to update or not, with or without detections (unlike
    COCOEvaluator's default, where an image without a detection does not count)."""

    def __init__(self, annotations=None, iou_thresh=0.5, as_written=False, label_index=None, device=None):
        if not isinstance(annotations, (list, tuple)) or not annotations:
            raise ValueError('annotations must be a non-empty list of images (id, event, stem, boxes, keep)')
        self.iou_thresh = float(iou_thresh)
        self.as_written = bool(as_written)
        self.label_index = None if label_index is None else int(label_index)
        if self.label_index is not None and self.label_index < 0:
            raise ValueError('label_index must not be negative')
        self.thr = widerface_thresholds()
        self._parse(annotations)
        self.ap = self.curve = self.faces = self.precision = self.recall = None
        self._start(device)

    # ------------------------------------------------------------------ ground truth (host)
    def _parse(self, annotations):
        self.image_ids = [a['id'] for a in annotations]
        self._img_ord = _annotation_index(annotations)
        box, kept, start, keep_len = [], [], [0], []
        for a in annotations:
            b = np.asarray(a['boxes'], np.float64).reshape(-1, 4)
            bits = np.zeros(len(b), np.uint8)
            lens = []
            for d, name in enumerate(DIFFICULTIES):
                idx = np.asarray(a['keep'][name], np.int64).reshape(-1)
                if len(idx) and (idx.min() < 0 or idx.max() >= len(b)):
                    raise ValueError('image %r: a %s keep index is outside its %d boxes' % (a['id'], name, len(b)))
                bits[idx] |= np.uint8(1 << d)
                lens.append(len(idx))
            box.append(b)
            kept.append(bits)
            keep_len.append(lens)
            start.append(start[-1] + len(b))
        self.gt_box = np.concatenate(box).reshape(-1, 4)
        self.gt_kept = np.concatenate(kept).astype(np.uint8)
        self.gt_start = np.array(start, np.int32)
        self.keep_len = np.array(keep_len, np.int32).reshape(len(annotations), 3)

    # ------------------------------------------------------------------ device state
    _STORE = ('det_box', 'det_score', 'det_img')                 # one class, and no img_mask
    _BUFS = ('gt_box', 'gt_start', 'gt_kept', 'keep_len', 'thr')
    _BUFS_STRUCT = 'WFEvalBufs'

    def _upload(self, d, up):
        G = len(self.gt_kept)
        d.gt_box = up(self.gt_box if G else np.zeros((1, 4)))
        d.gt_kept = up(self.gt_kept if G else np.zeros(1, np.uint8))
        d.gt_start, d.keep_len, d.thr = up(self.gt_start), up(self.keep_len), up(self.thr)

    def _desc(self):
        d = self._dev
        desc = d.lib.WFEvalDesc()
        desc.num_images, desc.num_gt, desc.det_capacity = len(self.image_ids), len(self.gt_kept), d.cap
        desc.num_thresholds = len(self.thr)
        desc.as_written = int(self.as_written)
        desc.label_index = -1 if self.label_index is None else self.label_index
        desc.iou_thresh = self.iou_thresh
        return desc

    # ------------------------------------------------------------------ accumulation
    def update(self, results):
        """results: tuple(predict_bboxes, meta_batch); predict_bboxes[i] is a list of [label, score, x, y, w, h] rows for
        image meta_batch[i]['image_id'] (what LFD.get_results / predict_for_single_image return).  With as_written the rows
        are quantised here, on the host, with the reference's own Python expressions."""
        predict_bboxes, meta_batch = self._split(results)
        ords = self._ordinals(meta_batch)
        rows = []
        for o, boxes in zip(ords, predict_bboxes):
            if self.as_written:
                rows.append((o, 0.001, 0.0, 0.0, 0.0, 0.0))
            for r in boxes:
                if self.label_index is not None and r[0] != self.label_index:
                    continue
                if self.as_written:
                    rows.append((o,) + _quantise_as_written(r))
                else:
                    rows.append((o, r[1], r[2], r[3], r[4], r[5]))
        if not ords:
            return
        self._seen.update(ords)
        if not rows:
            return
        self._append_rows('lfd_eval_wf_append_rows_f64', rows, 6)

    def update_resident(self, outputs, meta_batch):
        """Appends the kept boxes of an ops.DetectOutputs (LFD.detect / detect_resident) on the device: no .item(),
        .tolist(), .cpu() or synchronisation; the number of kept boxes is read from outputs.counts by the kernel, which also
        forms w = x2 - x1 + 1 and h in fp32 (the two roundings of LFD._pack) and, with as_written, does the quantisation and
        adds the dummy row.  The only host -> device traffic is the batch's image ordinals (pinned, asynchronous)."""
        ords = self._append_resident('lfd_eval_wf_append_dets_f32', outputs, meta_batch, lambda d, ords: (ords,), dummy_rows=1)
        self._seen.update(ords)

    # ------------------------------------------------------------------ evaluation
    def _run(self, keep_matches=False):
        """enqueue the score range, the grouping and the matching; returns the device tensors (no synchronisation)"""
        d = self._state()
        torch, lib = d.torch, d.lib
        I, T = len(self.image_ids), len(self.thr)
        with torch.cuda.device(d.dev):
            i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=d.dev)   # noqa: E731
            u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=d.dev)   # noqa: E731
            out = dict(det_start=i32(I + 1), det_index=i32(d.cap), det_gt=i32(d.cap), det_over=u8(d.cap), det_prop=i32(3, d.cap),
                       det_rec=i32(3, d.cap), det_flags=u8(d.cap) if keep_matches else None,
                       curve=torch.empty((3, T, 2), dtype=torch.int64, device=d.dev),
                       faces=torch.empty(3, dtype=torch.int64, device=d.dev),
                       minmax=torch.empty(2, dtype=torch.float64, device=d.dev))
            desc, bufs = self._desc(), self._bufs(**out)
            wb = lib.lib().lfd_eval_wf_workspace_bytes(C.byref(desc))
            if wb == 0:
                raise RuntimeError('WIDERFACEEvaluator: this problem size is not supported by the evaluation kernels')
            ws = torch.empty(wb, dtype=torch.uint8, device=d.dev)
            lib.check(lib.lib().lfd_eval_wf_match(C.byref(desc), C.byref(bufs), lib.ptr(ws), wb, lib.stream_ptr()),
                      'lfd_eval_wf_match')
        out['ws'] = ws
        return out

    def evaluate(self, keep_matches=False):
        """Runs the kernels on what update / update_resident accumulated and fills `curve` (int64 [3, 1000, 2]: proposals and
        recalled faces per difficulty and threshold), `faces` (int64 [3]), `precision`, `recall` (float64 [3, 1000]) and `ap`
        (float64 [3]), builds the display string, clears the accumulated detections and returns {'easy': ap, 'medium': ap,
        'hard': ap}.  keep_matches=True keeps the per-detection outcomes for `match_table()`."""
        T = len(self.thr)
        self._last = None
        stored = self._upper > 0
        if not stored:
            curve = np.zeros((3, T, 2), np.int64)
            faces = self.keep_len.astype(np.int64).sum(0)
            self._clear()
        else:
            d = self._state()
            torch = d.torch
            out = self._run(keep_matches)
            with torch.cuda.device(d.dev):
                flat = torch.cat([out['curve'].reshape(-1), out['faces'], d.state.long()]).cpu().numpy()   # the one D2H
            curve = flat[:6 * T].reshape(3, T, 2).copy()
            faces = flat[6 * T:6 * T + 3].copy()
            state = flat[6 * T + 3:]
            err = int(state[1])
            if keep_matches and not err:
                n = int(state[2])
                start = out['det_start'].cpu().numpy()
                ranked = np.repeat(np.diff(self.gt_start) > 0, np.diff(start))      # images without ground truth are not ranked
                self._last = dict(det_start=start, ranked=ranked)
                for k in ('det_index', 'det_gt', 'det_flags'):
                    self._last[k] = out[k][:n].cpu().numpy()
                for k in ('det_prop', 'det_rec'):
                    self._last[k] = out[k][:, :n].cpu().numpy()
            self._clear()
            if err:
                raise self._status_error(err)
        self.curve, self.faces = curve, faces
        self.precision, self.recall, self.ap = widerface_ap(curve, faces)
        self._eval_display_str = '\n' + ''.join('{:<10}:{:.5f}\n'.format(name + ' AP', self.ap[i]) for i, name in enumerate(DIFFICULTIES))
        return dict((name, float(self.ap[i])) for i, name in enumerate(DIFFICULTIES))

    def match_table(self, d=0):
        """After evaluate(keep_matches=True), for difficulty d (0 easy, 1 medium, 2 hard, or its name): dict of numpy arrays
        with one row per stored detection of an image that has ground truth, image-major and in rank order inside an image --
        `image` (ordinal in `image_ids`), `index` (index into the detection store: the insertion index, where update_resident
        with label_index also counts the rows of other labels, which keep their slot, and update does not), `rank`, `m` (first ground truth of
        maximal IoU, index inside the image's boxes), `over` (that IoU >= iou_thresh), `proposal` (bool) and `rec` (the
        running count of recalled faces)."""
        if self._last is None:
            raise RuntimeError('match_table: call evaluate(keep_matches=True) first')
        if d in DIFFICULTIES:
            d = DIFFICULTIES.index(d)
        L = self._last
        start, sel = L['det_start'], L['ranked']
        image = np.repeat(np.arange(len(start) - 1), np.diff(start))
        rank = np.arange(len(image)) - start[image]
        flags = L['det_flags'][sel]
        return dict(image=image[sel], index=L['det_index'][sel], rank=rank[sel], m=L['det_gt'][sel], over=(flags & 1).astype(bool),
                    proposal=((flags >> (1 + d)) & 1).astype(bool), rec=L['det_rec'][d][sel])
