"""tests/golden/resnet_cases.py -- the float64 reference, the seeded operands and the launch geometry for lfd_stem7_conv_f16
(csrc/stem7.hip: conv7x7 s2 p3, 3 -> 64, + bias + ReLU), shared by tests/test_gpu_stem7_exact.py and tests/test_gpu_resnet.py.
The generators return CPU tensors; no ctypes.

Instruments
  integer   frame values in {-2..2} (fp32 NCHW / fp16 NHWC), filter in {-1, 0, 1}, integer bias in [-8, 8]: every partial sum is
            an integer of magnitude <= 2 * 147 + 8 = 302 < 2048, exact in fp32 in any order and an fp16 value: bit equality.
  uint8     any byte v; the kernel sees x = half((v / 255 - 0.5) / 0.5) (fp32 arithmetic, csrc/stem7.hip load_px), a multiple of
            2^-18 with |x| <= 1.  Filter row co: 24 taps of +-2^-k(co), k in {0, 1, 2}, the rest 0; bias an integer in [-8, 8]
            times 2^-k.  Every partial sum is a multiple of 2^-(18 + k) below (24 + 8) 2^-k = 2^(5 - k): 23 bits, exact in fp32 in
            any order.  The one rounding left is fp32 -> fp16, which the float64 reference rounded once to fp16 reproduces
            bit for bit (ties included: both round to nearest even).
  gaussian  frame uniform in [-1, 1) and filter N(0, 0.1^2), both rounded to fp16; bias N(0, 0.1^2):
            |got - ref| <= 0.5005 ulp16(ref) + 2^-19 sum |x||w|, the project's per-launch tolerance.
"""
import torch

FMT_F32, FMT_F16, FMT_U8 = 0, 1, 2
FMT_NAMES = {FMT_F32: 'f32', FMT_F16: 'f16', FMT_U8: 'u8'}
TH, TW, MAX_WGS = 4, 32, 512           # csrc/stem7.hip: the tile in output pixels, the cap of the persistent grid
U8_TAPS = 24


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def ntiles(n, h, w):
    oh, ow = out_hw(h, w)
    return n * (-(-oh // TH)) * (-(-ow // TW))


# 3 frames of 121 x 975 -> maps of 61 x 488 = 16 x 16 tiles (the last row of tiles one pixel high, the last column 8 wide):
# 768 tiles on the 512 workgroups of the capped grid, 1.5 each -- every workgroup prefetches a second tile, half of them a
# tile of another image
WALK_SHAPE = (3, 121, 975)
SHAPES = {'corner': (1, 7, 7), 'ragged': (2, 37, 53), 'pixel': (1, 1, 1), 'walk': WALK_SHAPE}


def conv_ref(x, w, bias, stride=2, dtype=torch.float64):
    """x NHWC [n, h, w, cin], w OIHW with an odd kernel (pad = ks // 2): ks * ks shifted matmuls over the zero-padded input, no
    conv call (tests/golden/conv_cases.py conv_ref for any odd ks) -> [n, oh, ow, cout] + bias, no ReLU"""
    n, h, wd, cin = x.shape
    cout, _, ks, _ = w.shape
    pad = ks // 2
    oh, ow = (h + 2 * pad - ks) // stride + 1, (wd + 2 * pad - ks) // stride + 1
    xp = torch.zeros((n, h + 2 * pad, wd + 2 * pad, cin), dtype=dtype, device=x.device)
    xp[:, pad:pad + h, pad:pad + wd] = x.to(dtype)
    wt = w.to(dtype).to(x.device)
    out = torch.zeros((n * oh * ow, cout), dtype=dtype, device=x.device)
    for ky in range(ks):
        for kx in range(ks):
            xs = xp[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride]
            out += xs.reshape(-1, cin) @ wt[:, :, ky, kx].t()
    return out.reshape(n, oh, ow, cout) + bias.to(dtype).to(x.device)


def normalize_u8(codes):
    """what the kernel sees of a uint8 frame: its expression, in fp32, rounded to fp16"""
    return ((codes.float() / 255.0 - 0.5) / 0.5).half()


def int_operands(shape, seed):
    """-> (values NHWC float [n, h, w, 3], w [64, 3, 7, 7], b [64]), integers"""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (n, h, w, 3), generator=g).float()
    wt = torch.randint(-1, 2, (64, 3, 7, 7), generator=g).float()
    b = torch.randint(-8, 9, (64,), generator=g).float()
    b[b == 0] = 3.0
    return x, wt, b


def u8_operands(shape, seed):
    """-> (codes uint8 NHWC [n, h, w, 3], w, b) as the module docstring says"""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    wt = torch.zeros(64, 147)
    for co in range(64):
        taps = torch.randperm(147, generator=g)[:U8_TAPS]
        wt[co, taps] = (torch.randint(0, 2, (U8_TAPS,), generator=g) * 2 - 1).float()
    scale = torch.pow(2.0, -torch.randint(0, 3, (64,), generator=g).float())
    b = torch.randint(-8, 9, (64,), generator=g).float()
    b[b == 0] = -5.0
    return codes, (wt * scale[:, None]).reshape(64, 3, 7, 7), b * scale


def gauss_operands(shape, seed):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, h, w, 3, generator=g) * 2 - 1).half().float()
    wt = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).half().float()
    return x, wt, torch.randn(64, generator=g) * 0.1


def to_frame(values, fmt):
    """NHWC float values -> the frame tensor of format fmt (fp32 NCHW / fp16 NHWC); uint8 codes pass through"""
    if fmt == FMT_U8:
        assert values.dtype == torch.uint8
        return values.contiguous()
    return values.permute(0, 3, 1, 2).contiguous() if fmt == FMT_F32 else values.half().contiguous()


def ulp16(v, floor=2.0 ** -14):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp(min=floor))) - 10)
