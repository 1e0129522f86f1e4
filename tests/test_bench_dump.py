"""bench.py --dump-outputs on the host: the files a run writes from a step's ops.DetectOutputs (no device)."""
import os

import numpy as np
import torch

import bench


def _outputs(n, cap, kept):
    g = torch.Generator().manual_seed(0)
    return {'dets': torch.rand(n, cap, 5, generator=g), 'labels': torch.randint(0, 3, (n, cap), generator=g, dtype=torch.int32),
            'cand': torch.randint(0, 99, (n, cap), generator=g, dtype=torch.int32),
            'point': torch.randint(0, 99, (n, cap), generator=g, dtype=torch.int32),
            'counts': torch.tensor([[k + 5, k, 0, k + 5] for k in kept], dtype=torch.int32)}


def test_dump_outputs_keeps_valid_rows_and_zeroes_the_rest(tmp_path):
    last = _outputs(3, 16, [4, 0, 16])
    bench.dump_outputs(last, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(k + '.npy' for k in bench.DUMP_KEYS)
    got = {k: np.load(os.path.join(tmp_path, k + '.npy')) for k in bench.DUMP_KEYS}
    assert got['dets'].dtype == np.float32 and got['dets'].shape == (3, 16, 5)
    assert all(got[k].dtype == np.float64 and got[k].shape == (3, 16) for k in ('labels', 'cand', 'point'))
    np.testing.assert_array_equal(got['counts'], last['counts'].numpy())
    for i, k in enumerate([4, 0, 16]):
        np.testing.assert_array_equal(got['dets'][i, :k], last['dets'][i, :k].numpy())
        assert not got['dets'][i, k:].any()
        for name in ('labels', 'cand', 'point'):
            np.testing.assert_array_equal(got[name][i, :k], last[name][i, :k].numpy())
            assert not got[name][i, k:].any()


def test_dump_outputs_stays_within_64_mb(tmp_path):
    cap = 600000                      # --max-candidates far above what 64 MB holds for a batch of 8
    last = _outputs(8, cap, [cap] * 8)
    bench.dump_outputs(last, str(tmp_path))
    total = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path))
    assert total <= 64 << 20
    d = np.load(os.path.join(tmp_path, 'dets.npy'))
    assert 0 < d.shape[1] < cap
    np.testing.assert_array_equal(d, last['dets'][:, :d.shape[1]].numpy())
