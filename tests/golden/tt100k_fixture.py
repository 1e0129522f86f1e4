"""Reads tests/golden/ref_tt100k_eval.npz (written by make_golden_tt100k_eval.py from the reference's own eval_annos) and turns
it into the inputs of lfd_amd.evaluation.TT100KEvaluator and of tt100k_eval_oracle.py.  Shared by the host and the GPU tests."""
import json
import os

import numpy as np

import tt100k_eval_oracle as oracle

HERE = os.path.dirname(os.path.abspath(__file__))


class Fixture(object):

    def __init__(self, z):
        self.names = [str(n) for n in z['names']]              # label index -> name
        self.cat_names = [str(n) for n in z['cat_names']]      # the index space of gt_cat; labels come first, so label == index
        self.type45 = [str(n) for n in z['type45']]
        self.images = [str(n) for n in z['image_ids']]
        self.gt_box, self.gt_cat, self.gt_img = z['gt_box'], z['gt_cat'], z['gt_img']
        self.det, self.det_label, self.det_img = z['det'], z['det_label'], z['det_img']
        self.num_groups = int(z['num_groups'])
        self.results_json = str(z['results_json'])
        self._z = z
        assert self.cat_names[:len(self.names)] == self.names and self.det.dtype == np.float32 and self.gt_box.dtype == np.float64

    def params(self, g):
        return json.loads(str(self._z['g%d_params' % g]))

    def expected(self, g):
        return dict((k, self._z['g%d_%s' % (g, k)]) for k in ('right', 'num_detections', 'num_ground_truth', 'accuracy', 'recall',
                                                             'det_code', 'gt_missed', 'report'))

    def in_types(self, types):
        return None if types is None else np.array([n in types for n in self.cat_names])

    def annotations(self):
        imgs = dict()
        for i, iid in enumerate(self.images):
            objs = [dict(bbox=dict(xmin=float(b[0]), ymin=float(b[1]), xmax=float(b[2]), ymax=float(b[3])), category=self.cat_names[c])
                    for b, c in zip(self.gt_box[self.gt_img == i], self.gt_cat[self.gt_img == i])]
            imgs[iid] = dict(id=iid, objects=objs)
        return dict(imgs=imgs, types=list(self.cat_names))

    def meta(self):
        """ids that are all digits arrive as ints: the evaluator looks them up as str(...)"""
        return [dict(image_id=int(i) if i.isdigit() else i) for i in self.images]

    def rows(self):
        """per image the [label, score, x, y, w, h] rows LFD.get_results makes of the fp32 detections (torch fp32 on the CPU)"""
        import torch
        out = []
        for i in range(len(self.images)):
            sel = self.det_img == i
            if not sel.any():
                out.append([])
                continue
            d = torch.from_numpy(np.ascontiguousarray(self.det[sel])).clone()
            d[:, 2] = d[:, 2] - d[:, 0] + 1
            d[:, 3] = d[:, 3] - d[:, 1] + 1
            rows = torch.cat([torch.from_numpy(self.det_label[sel].astype(np.float32))[:, None], d[:, [4, 0, 1, 2, 3]]], dim=1).tolist()
            out.append([[int(r[0])] + r[1:] for r in rows])
        return out

    def oracle_images(self):
        box, score = oracle.detections_from_f32(self.det)
        return [(self.gt_box[self.gt_img == i], self.gt_cat[self.gt_img == i], box[self.det_img == i], self.det_label[self.det_img == i],
                 score[self.det_img == i]) for i in range(len(self.images))]


def load():
    return Fixture(np.load(os.path.join(HERE, 'ref_tt100k_eval.npz'), allow_pickle=False))
