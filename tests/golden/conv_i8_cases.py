"""tests/golden/conv_i8_cases.py -- case table, seeded operands and the float64 oracle for csrc/conv_i8.hip
(lfd_conv2d_nhwc_i8: NHWC int8 conv, ks 1 | 3, stride 1 | 2, cin and cout in {64, 128}, requantising epilogue), in the manner
of tests/golden/conv256_cases.py.

Operands: x and the filter are FULL-RANGE int8 in [-127, 127], drawn independently per element, so the filter is asymmetric in
output channel, input channel and tap; |acc| <= 9 * 128 * 127^2 < 2^31.  The oracle sums ks * ks shifted matmuls in float64 (every
partial sum is an integer below 2^53: exact, = the int64 sum), no conv call, then applies the epilogue of DESIGN 4j in float64:
    v = acc * mult[co] + biasq[co];  res: v += q_res * res_mult;  relu: v = max(v, 0);  q = clamp(rint(v), -127, 127)
    out_f16 = half(v * out_scale)

Two instruments:
  (a) exact_constants: mult[co] = 2^-k or 2^-(k+1), biasq and res_mult integer multiples of 2^-k.  With |acc| < 2^22 (asserted;
      a sum of K products of variance (127 * 128 / 3)^2 has sigma = 5419 sqrt(K) <= 184e3, so 2^22 is a > 22-sigma event) every
      value of the epilogue is an integer multiple of 2^-(k+1) below 2^24 of them: exact in fp32 whatever the order, ties
      (exact .5) included.  out_scale is a power of two.  The kernel must match bit for bit.
  (b) random_constants: arbitrary fp32 mult / biasq / res_mult / out_scale.  The kernel's fp32 epilogue differs from the float64
      one by a few 2^-24 relative, so q may differ only where the oracle's v lies within NEAR_TIE of a half-integer (there by
      +-1); such outputs must be at most NEAR_TIE_CAP of a case -- for a continuous v that share is about 2 * NEAR_TIE = 0.2 % --
      which tests/test_conv_i8_host.py checks on the oracle alone for every case.

Launch geometry restated (csrc/conv_i8.hip): tiles of TH x 16 output pixels, TH = 8 at stride 1 and 4 at stride 2, every output
channel in one workgroup, grid = min(ntiles, 1024); workgroup b walks tiles b, b + grid, ... of the order (image, tile row,
tile column)."""
import collections
import functools
import math

import torch

QMAX = 127
TW, MAX_WORKGROUPS = 16, 1024
NEAR_TIE, NEAR_TIE_CAP = 1e-3, 0.01

KEYS = [(cin, cout, ks, stride) for cin in (64, 128) for cout in (64, 128) for ks in (1, 3) for stride in (1, 2)]

Case = collections.namedtuple('Case', 'cin cout ks stride kind n h w')        # h, w: the INPUT map
Consts = collections.namedtuple('Consts', 'mult biasq res_mult out_scale')


def tile_h(stride):
    return 8 if stride == 1 else 4


def out_hw(h, w, ks, stride):
    pad = ks // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def launch(c):
    """-> (tiles_x, tiles_y, ntiles, grid) of lfd_conv2d_nhwc_i8"""
    oh, ow = out_hw(c.h, c.w, c.ks, c.stride)
    tx, ty = -(-ow // TW), -(-oh // tile_h(c.stride))
    nt = c.n * tx * ty
    return tx, ty, nt, min(nt, MAX_WORKGROUPS)


def edge_shape(stride):
    """input map whose output is one pixel past a tile in each direction"""
    return 2, stride * tile_h(stride) + 1, stride * TW + 1


def walk_shape(stride):
    """images whose OUTPUT is (TH + 1) x (2 TW + 1) -- 2 x 3 tiles: two full, a ragged right column of one pixel, a ragged bottom
    row of one pixel under each -- just enough of them for 1.5 tiles per workgroup of the capped grid: workgroups 0 .. 511 run
    two tiles, the others one, and a workgroup's two tiles lie in different images at different places (1024 = 4 mod 6)."""
    n = -(-(3 * MAX_WORKGROUPS) // (2 * 6))
    return n, stride * tile_h(stride) + 1, stride * 2 * TW + 1


def small_cases():
    return [Case(*k, kind, *m) for k in KEYS
            for kind, m in (('pixel', (1, 1, 1)), ('small', (2, 5, 11)), ('edge', edge_shape(k[3])))]


def walk_cases():
    """one walk map per (ks, stride), 64 -> 64 channels"""
    return [Case(64, 64, ks, stride, 'walk', *walk_shape(stride)) for ks in (1, 3) for stride in (1, 2)]


def random_cases():
    """(b): every key on the small and the edge map"""
    return [c for c in small_cases() if c.kind != 'pixel']


def case_id(c):
    return '%dto%d_k%ds%d_%s_%dx%dx%d' % (c.cin, c.cout, c.ks, c.stride, c.kind, c.n, c.h, c.w)


def case_seed(c):
    return sum(int(v) * p for v, p in zip((c.cin, c.cout, c.ks, c.stride, c.n, c.h, c.w), (7, 11, 3, 5, 17, 19, 23))) + 8


def _randint8(shape, seed):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-QMAX, QMAX + 1, tuple(shape), generator=g, dtype=torch.int16).to(torch.int8)


@functools.lru_cache(maxsize=2)
def operands(c):
    """-> (x [n,h,w,cin], w [cout,cin,ks,ks], res [n,oh,ow,cout]) int8 CPU tensors, full range"""
    s = case_seed(c)
    oh, ow = out_hw(c.h, c.w, c.ks, c.stride)
    return (_randint8((c.n, c.h, c.w, c.cin), s), _randint8((c.cout, c.cin, c.ks, c.ks), s + 100003),
            _randint8((c.n, oh, ow, c.cout), s + 300007))


def _k0(c):
    """2^-k0 brings an accumulator of sigma 5419 sqrt(K) to a sigma of about 64 quantised steps: both clamps are reached"""
    return int(round(math.log2(5419.0 * math.sqrt(c.ks * c.ks * c.cin) / 64.0)))


def exact_constants(c):
    """(a): mult 2^-k0 on even channels and 2^-(k0 + 1) on odd ones, biasq = a half-integer in [-24, 24] plus up to three steps of
    2^-k0 (so that exact ties occur), res_mult = 3 / 4, out_scale = 2^-3"""
    k0 = _k0(c)
    ch = torch.arange(c.cout)
    mult = torch.where(ch % 2 == 0, torch.tensor(2.0 ** -k0), torch.tensor(2.0 ** -(k0 + 1))).float()
    g = torch.Generator().manual_seed(case_seed(c) + 200003)
    biasq = (torch.randint(-48, 49, (c.cout,), generator=g).float() * 0.5 + 2.0 ** -k0 * torch.randint(-3, 4, (c.cout,), generator=g).float())
    return Consts(mult, biasq.float(), 0.75, 0.125)


def random_constants(c):
    """(b): arbitrary fp32 constants of the same magnitudes"""
    g = torch.Generator().manual_seed(case_seed(c) + 400009)
    mult = (2.0 ** -_k0(c) * (0.6 + 0.9 * torch.rand(c.cout, generator=g))).float()
    biasq = ((torch.rand(c.cout, generator=g) * 2 - 1) * 24).float()
    res_mult = float((0.3 + 0.6 * torch.rand(1, generator=g)).float())
    out_scale = float((0.02 + 0.05 * torch.rand(1, generator=g)).float())
    return Consts(mult, biasq, res_mult, out_scale)


def acc_ref(x, w, stride):
    """exact integer conv as float64 [n, oh, ow, cout]: ks * ks shifted matmuls over the zero-padded input, on x's device"""
    n, h, wd, cin = x.shape
    cout, cin_w, ks, _ = w.shape
    assert cin_w == cin and ks in (1, 3)
    pad = ks // 2
    oh, ow = out_hw(h, wd, ks, stride)
    xp = torch.zeros((n, h + 2 * pad, wd + 2 * pad, cin), dtype=torch.float64, device=x.device)
    xp[:, pad:pad + h, pad:pad + wd] = x.double()
    wt = w.double()
    out = torch.zeros((n * oh * ow, cout), dtype=torch.float64, device=x.device)
    for ky in range(ks):
        for kx in range(ks):
            xs = xp[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride]
            out += xs.reshape(-1, cin) @ wt[:, :, ky, kx].t()
    return out.reshape(n, oh, ow, cout)


def epilogue_ref(acc, k, res=None, relu=False):
    """float64 epilogue on an accumulator map -> (v, q int8, v * out_scale float64)"""
    v = acc * k.mult.double().to(acc.device) + k.biasq.double().to(acc.device)
    if res is not None:
        v = v + res.double() * float(torch.tensor(k.res_mult, dtype=torch.float32).double())
    if relu:
        v = v.clamp(min=0)
    q = torch.round(v).clamp(-QMAX, QMAX).to(torch.int8)
    return v, q, v * float(torch.tensor(k.out_scale, dtype=torch.float32).double())


def near_tie(v):
    """outputs of the float64 oracle within NEAR_TIE of a half-integer (where the fp32 epilogue may round the other way)"""
    return ((v - torch.floor(v)) - 0.5).abs() < NEAR_TIE


def f16_ulp(ref):
    """spacing of fp16 at |ref| (float64 tensor): 2^(floor(log2 |ref|) - 10), 2^-24 below the smallest normal"""
    e = torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=ref.device), e - 10)
