"""INT8 deployment plan: the fp16 engine's stem and neck + head around residual stages that run in int8 on
csrc/conv_i8.hip -- what the reference gets from a TensorRT engine built with precision_mode='int8'
(lfd/deployment/tensorrt/build_engine.py:22-126).  lfd_amd/deployment.py is the public interface.

Split of the network: stem = the parent plan's fp16 launches; one quantise launch; every conv of the residual stages, identity
branches included, one lfd_conv2d_nhwc_i8 launch each (layer by layer, the default); a conv whose output is a pyramid tap also
stores the un-requantised fp16 map the parent's head kernels read.  Int8Plan(..., fused=True) runs the same layer list through
lower_fused(): a stage-entry block's two stride-2 convs as one lfd_conv2d_downsample_nhwc_i8 launch, a 64-channel block without
a downsample as one lfd_block_i8_fused launch (csrc/block_i8.hip), the rest as before -- the same bits in every tensor the route
still writes (the int8 map between a fused block's convs stays on chip and has no buffer).  fused='full' additionally runs a
whole 64-channel stage-entry block as one lfd_entry_i8_fused launch (csrc/entry_i8.hip); the first of them reads the fp16 stem
map and quantises on the way in, so the quantise launch and the int8 copy of the stem map are gone as well.  block128=True (with
either fused route) runs every 128-channel block without a downsample as one lfd_block128_i8_fused launch
(csrc/block128_i8.hip), the same bits again.  stem_int8=True (with every route) lets the stem launch write the int8 map itself
(lfd_stem_conv_i8 / lfd_stem_faster_fused_i8) for the frame formats in Int8Plan.stem_int8_formats: no fp16 stem map, no quantise
launch, and the first 'entry' launch reads int8 -- the same bits once more.

Numeric contract (symmetric, range [-127, 127], no zero points):
  weights      BN-folded fp32 (engine.fold_conv_norm, channels zero-padded to 64 / 128); per output channel
               s_w[co] = max|w[co]| / 127 (a zero row: 1), q_w = clamp(rint(w / s_w))
  activations  one scale per tensor t (the stem output, or a conv's output after bias, residual add and ReLU):
               s_t = amax_t / 127 (amax_t == 0: 1), amax_t the largest |value| over all calibration batches of the fp16 pass
  constants    float64 -> fp32: mult[co] = s_in s_w[co] / s_out, biasq[co] = b[co] / s_out, res_mult = s_res / s_out
  epilogue     include/lfd_hip.h, lfd_conv2d_nhwc_i8
There is no fp16 fallback: a model outside the coverage raises engine.Unsupported."""
import collections
import ctypes as C

import numpy
import torch
import torch.nn.functional as F

from . import _lib, engine, engine_resnet, netdesc, ops
from ._lib import check, lib, ptr, stream_ptr

QMAX = 127
STEM = 'stem'       # name of the calibrated tensor in front of the stages


def pad_channels_i8(c, what):
    """the int8 kernels are instantiated for 64 and 128 channels: 32 / 48 run zero-padded to 64"""
    if c <= 64:
        return 64
    if c <= 128:
        return 128
    engine._unsupported('more than 128 channels (%d) in %s: the INT8 mode has kernels for bodies of up to 128 channels' % (c, what))


def weight_scales(w):
    """folded fp32 OIHW weight -> (s_w [cout] float64, q_w int8 OIHW): s_w = max|w[co]| / 127, 1 for a zero row"""
    amax = w.detach().double().abs().flatten(1).max(1)[0]
    s_w = torch.where(amax > 0, amax / QMAX, torch.ones_like(amax))
    q = torch.round(w.detach().double() / s_w.view(-1, 1, 1, 1)).clamp(-QMAX, QMAX).to(torch.int8)
    return s_w, q


def act_scale(amax):
    """amax of a tensor -> its scale (float64 arithmetic on Python floats)"""
    return float(amax) / QMAX if amax > 0 else 1.0


def epilogue_constants(s_in, s_w, bias, s_out, s_res=None):
    """(mult [cout] fp32, biasq [cout] fp32, res_mult float): computed in float64, stored as fp32"""
    mult = (s_w.double() * s_in / s_out).float()
    biasq = (bias.double() / s_out).float()
    res_mult = float(torch.tensor(s_res / s_out, dtype=torch.float64).float()) if s_res is not None else 0.0
    return mult, biasq, res_mult


def _pad_to(w, b, cout, cin):
    if (cout, cin) == tuple(w.shape[:2]):
        return w, b
    wp = torch.zeros((cout, cin) + tuple(w.shape[2:]), dtype=w.dtype, device=w.device)
    wp[:w.shape[0], :w.shape[1]] = w
    bp = torch.zeros(cout, dtype=b.dtype, device=b.device)
    bp[:b.shape[0]] = b
    return wp, bp


class ConvI8(object):
    """one lfd_conv2d_nhwc_i8 launch over symbolic int8 buffer ids; name = the calibrated tensor it produces"""
    __slots__ = ('name', 'cin', 'cout', 'cout_real', 'ks', 'stride', 'relu', 'src', 'dst', 'res', 'tap', 'src_name', 'res_name',
                 'ref_w', 'ref_b', 'q_w', 's_w', 'w', 'w16', 'mult', 'biasq', 'res_mult', 's_in', 's_out', 's_res')


# a launch of the fused route over indices into the layer list: 'conv' (i,) one lfd_conv2d_nhwc_i8; 'pair' (downsample, conv1) one
# lfd_conv2d_downsample_nhwc_i8 (csrc/conv_i8.hip); 'block' (conv1, conv2) one lfd_block_i8_fused; 'entry' (downsample, conv1, conv2) one
# lfd_entry_i8_fused (the 'full' route only); 'block128' (conv1, conv2) one lfd_block128_i8_fused (the block128 option only)
Launch = collections.namedtuple('Launch', 'kind layers')
PAIR_KEYS = ((64, 64), (64, 128), (128, 128))     # (cin, cout) of lfd_conv2d_downsample_nhwc_i8
ROUTES = ('layers', 'fused', 'full')              # Int8Plan.route for fused = False, True, 'full'


def lower_fused(layers, entry=False, block128=False):
    """the plan's layer list -> the launch list of the fused route (a pure function of the layers' shapes and buffer ids).
    entry block (downsample 1x1 s2, conv1 3x3 s2 of the same input, conv2 adding the downsample): 'pair' + 'conv';
    block of two 3x3 s1 convs of 64 (padded) channels whose second adds the first's input: 'block'; everything else: 'conv'.
    entry=True (the 'full' route): an entry block of 64 -> 64 (padded) channels whose conv2 is no tap and whose two intermediate
    maps nothing else reads is one 'entry' launch.
    block128=True: a block of two 3x3 s1 convs of 128 (padded) channels under the conditions of 'block' (conv2 may be a tap) is
    one 'block128' launch; with block128=False it stays two 'conv' launches."""
    def reads(buf, but):
        return [j for j, c in enumerate(layers) if j not in but and (c.src == buf or c.res == buf)]

    out, i = [], 0
    while i < len(layers):
        a = layers[i]
        b = layers[i + 1] if i + 1 < len(layers) else None
        c = layers[i + 2] if i + 2 < len(layers) else None
        if b is not None and c is not None and (a.ks, a.stride, a.relu, a.res, a.tap) == (1, 2, False, None, None) \
                and (b.ks, b.stride, b.relu, b.res, b.tap) == (3, 2, True, None, None) and b.src == a.src \
                and (a.cin, a.cout) == (b.cin, b.cout) and (a.cin, a.cout) in PAIR_KEYS and c.src == b.dst and c.res == a.dst:
            if entry and (a.cin, a.cout) == (64, 64) and (c.ks, c.stride, c.relu, c.tap) == (3, 1, True, None) \
                    and c.cin == c.cout == 64 and not reads(a.dst, (i + 2,)) and not reads(b.dst, (i + 2,)):
                out.append(Launch('entry', (i, i + 1, i + 2)))
                i += 3
                continue
            out.append(Launch('pair', (i, i + 1)))
            i += 2
            continue
        if b is not None and (a.ks, a.stride, a.relu, a.res, a.tap) == (3, 1, True, None, None) \
                and (b.ks, b.stride, b.relu) == (3, 1, True) and a.cin == a.cout == b.cin == b.cout \
                and a.cin in ((64, 128) if block128 else (64,)) \
                and b.src == a.dst and b.res == a.src and not reads(a.dst, (i + 1,)):
            out.append(Launch('block' if a.cin == 64 else 'block128', (i, i + 1)))
            i += 2
            continue
        out.append(Launch('conv', (i,)))
        i += 1
    return out


def check_model(model):
    """the INT8 mode covers the LFD models of the fused fp16 plan with stage convs of up to 128 (padded) channels; everything
    else is named here (the plan's own constructor refuses the rest)"""
    kind = type(model).__name__
    if kind != 'LFD':
        engine._unsupported('the INT8 mode covers LFD models only, not %s' % kind)
    if not engine_resnet.is_lfd_resnet(model._backbone):
        engine._unsupported('the INT8 mode covers the LFDResNet backbone only, not %s' % type(model._backbone).__name__)
    if type(model._neck).__name__ != 'SimpleNeck':
        engine._unsupported('the INT8 mode covers SimpleNeck only, not %s' % type(model._neck).__name__)
    if type(model._head).__name__ != 'LFDHead' or model._head._conv_kernel_size != 1:
        engine._unsupported('the INT8 mode covers an LFDHead of 1x1 convs only, not %s' % type(model._head).__name__)
    if model.precision != 'fp16':
        engine._unsupported("the INT8 mode keeps the stem and the head on the 'fp16' kernels; the model's precision is %r"
                            % (model.precision,))
    for m in model._backbone.modules():
        if isinstance(m, torch.nn.Conv2d) and max(m.in_channels, m.out_channels) > 128:
            engine._unsupported('more than 128 channels (conv %d -> %d) in the backbone: the INT8 mode has kernels for bodies of '
                                'up to 128 channels' % (m.in_channels, m.out_channels))


class Int8Plan(engine.EnginePlan):
    """engine.EnginePlan whose residual stages are int8 launches.  Built without scales (layers, folded and quantised weights);
    calibrate() measures the amax of every named tensor in fp16 (calibrate_histograms(): its magnitude histogram, for the
    clipping rules of lfd_amd/calibration.py), set_scales() turns one value per tensor into the launches' constants."""

    def __init__(self, backbone, neck=None, head=None, device=None, fused=False, block128=False, stem_int8=False):
        self.layers = []
        self.scales = None
        if not any(fused is v for v in (False, True)) and fused != 'full':
            raise ValueError("Int8Plan: fused must be False, True or 'full', not %r" % (fused,))
        if not any(block128 is v for v in (False, True)):
            raise ValueError('Int8Plan: block128 must be False or True, not %r' % (block128,))
        if not any(stem_int8 is v for v in (False, True)):
            raise ValueError('Int8Plan: stem_int8 must be False or True, not %r' % (stem_int8,))
        if block128 and fused is False:
            raise ValueError("Int8Plan: block128=True needs fused=True or fused='full': the layer-by-layer route has no fused "
                             'launches')
        self.block128 = block128                              # 128-channel blocks as one lfd_block128_i8_fused launch each
        self.stem_int8 = stem_int8                            # the stem launch writes int8 buffer 0 where it can
        self.stem_int8_formats = frozenset()                  # in_format values for which it does (filled by _build_stages)
        self.front = None                                     # log of the launches in front of the stages (run_stem), not state
        self.fused = fused                                    # truthy for both fused routes
        self.route = ROUTES[2 if fused == 'full' else int(fused)]
        self.launches = None                                  # the fused routes' launch list (lower_fused), else None
        self.entry_f16 = None                                 # index of the 'entry' launch that reads the fp16 stem map
        super().__init__(backbone, neck, head, device)
        self.stem_channels_real = netdesc.backbone_layers(backbone).stem[-1].conv.out_channels

    # ---- lowering
    def _build_stages(self, blocks, cur, new_buf):
        dev = self.device
        self.taps, self.tap_channels, self.tap_ready_after = [], [], []
        self.stage_in = cur                                   # fp16 buffer the stem launches leave their output in
        c_in = pad_channels_i8(self.buf_channels[cur], 'the stem')
        self.qbuf_channels = {0: c_in}
        self.qbuf_scale = {0: self.buf_scale[cur]}
        self.tensor_names = [STEM]
        self.stem_int8_formats = self._stem_int8_formats(cur) if self.stem_int8 else frozenset()

        def add(src, src_name, lay, name, relu, res=None, res_name=None, tap=False):
            c = ConvI8()
            c.name, c.ks, c.stride, c.relu = name, lay.ks, lay.stride, bool(relu)
            c.cin = pad_channels_i8(lay.conv.in_channels, name)
            c.cout = pad_channels_i8(lay.conv.out_channels, name)
            c.cout_real = lay.conv.out_channels
            if lay.ks not in (1, 3) or lay.stride not in (1, 2) or lay.conv.padding[0] != lay.ks // 2 or lay.conv.groups != 1 \
                    or lay.conv.dilation[0] != 1 or not ops.conv2d_i8_supported(c.cin, c.cout, lay.ks, lay.stride):
                engine._unsupported('%s: no int8 kernel for a %d -> %d conv, kernel %d, stride %d'
                                    % (name, lay.conv.in_channels, lay.conv.out_channels, lay.ks, lay.stride))
            if c.cin != self.qbuf_channels[src]:
                engine._unsupported('%s: %d input channels behind a %d-channel tensor' % (name, c.cin, self.qbuf_channels[src]))
            w, b = engine._fold_conv_norm(lay.conv, lay.norm)
            c.ref_w, c.ref_b = _pad_to(w, b, c.cout, c.cin)
            c.s_w, c.q_w = weight_scales(c.ref_w)
            c.w = ops.pack_conv_weight_i8(c.q_w).to(dev)
            c.w16 = None                                      # fp16 fragment order of ref_w, packed when calibrate() needs it
            c.ref_b = c.ref_b.to(dev)
            c.src, c.res, c.src_name, c.res_name = src, res, src_name, res_name
            c.dst = len(self.qbuf_channels)
            self.qbuf_channels[c.dst] = c.cout
            self.qbuf_scale[c.dst] = self.qbuf_scale[src] * lay.stride
            c.tap = None
            if tap:                                           # the fp16 map engine.EnginePlan.run_head reads
                c.tap = new_buf()
                self.buf_channels[c.tap] = c.cout
                self.buf_scale[c.tap] = self.qbuf_scale[c.dst]
            c.mult = c.biasq = None
            self.layers.append(c)
            self.tensor_names.append(name)
            return c.dst

        q, q_name = 0, STEM
        for blk in blocks:
            base = 'stage%d.block%d' % (blk.stage, blk.index)
            ident, ident_name = q, q_name
            if blk.downsample is not None:
                ident_name = base + '.downsample'
                ident = add(q, q_name, blk.downsample, ident_name, False)
            y, y_name = q, q_name
            for ci, lay in enumerate(blk.convs):
                last = ci == len(blk.convs) - 1
                if not lay.relu:
                    engine._unsupported('activation must be ReLU')
                name = '%s.conv%d' % (base, ci + 1)
                y = add(y, y_name, lay, name, True, res=ident if last else None, res_name=ident_name if last else None,
                        tap=blk.tap and last)
                y_name = name
            if self.qbuf_channels[ident] != self.qbuf_channels[y]:
                engine._unsupported('%s: residual of %d channels added to %d' % (base, self.qbuf_channels[ident], self.qbuf_channels[y]))
            q, q_name = y, y_name
            if blk.tap:
                self.taps.append(self.layers[-1].tap)
                self.tap_channels.append(blk.convs[-1].conv.out_channels)
                self.tap_ready_after.append(len(self.convs) + len(self.layers))
        self.unwritten = frozenset()                          # int8 buffers no launch of this plan's route writes
        if self.fused:
            self.launches = lower_fused(self.layers, entry=self.route == 'full', block128=self.block128)
            gone = [self.layers[la.layers[0]].dst for la in self.launches if la.kind in ('block', 'block128')]
            for k, la in enumerate(self.launches):
                if la.kind != 'entry':
                    continue
                gone += [self.layers[i].dst for i in la.layers[:2]]       # the identity map and conv1's map stay on chip
                # the entry launch behind the stem takes the fp16 stem map itself: no quantise launch, no int8 copy of it
                if self.layers[la.layers[0]].src == 0 and ops.entry_i8_fused_supported(1, self.buf_channels[cur]) \
                        and not [c for j, c in enumerate(self.layers) if j not in la.layers[:2] and 0 in (c.src, c.res)]:
                    self.entry_f16 = k
                    gone.append(0)
            if self.stem_int8_formats:                        # the stem launch writes int8 buffer 0 for those formats
                gone = [b for b in gone if b != 0]
            self.unwritten = frozenset(gone)
            done = dict((la.layers[-1], len(self.convs) + k + 1) for k, la in enumerate(self.launches))
            self.tap_ready_after = [done[i] for i, c in enumerate(self.layers) if c.tap is not None]

    def _stem_int8_formats(self, cur):
        """frame formats (in_format of lfd_stem_conv_f16) for which the launch that writes the stem map `cur` has an int8-output
        form: a pure function of the model.  RGB stems whose last launch is the 'fast' unit (64 stored channels -- a 48-channel
        stem runs zero-padded to 64 and its padded channels quantise to 0 -- with the 1x1 tail) or the one-launch 'faster' stem
        (NHWC fp16 / uint8 frames; NCHW fp32 frames run its two-kernel form).  Gray models and 32-channel stems: none."""
        if self.input_channels != 3 or self.buf_channels[cur] != self.qbuf_channels[0]:
            return frozenset()
        c0 = self.stem_first[0]
        if self.stem_fused is not None:
            if self.stem_fused[-1] != cur or self.convs:
                return frozenset()
            return frozenset(f for f in (1, 2) if ops.stem_faster_fused_i8_supported(f, c0))
        if self.convs or cur != self.stem_out:                # further stem launches behind the first unit
            return frozenset()
        return frozenset(f for f in (0, 1, 2) if ops.stem_conv_i8_supported(f, c0, self.stem_first[3] is not None))

    def int8_launches(self):
        """int8 launches of the stages per forward.  Not counted: the launches in front of them -- the stem's and the quantise
        launch, which is gone under fused='full' and, with stem_int8=True, for every frame format in stem_int8_formats (the
        launch list and this count do not depend on stem_int8)"""
        return len(self.launches) if self.fused else len(self.layers)

    # ---- calibration (offline: fp16 kernels where they exist, torch otherwise)
    def _calibration_walk(self, batches, see):
        """the stem launches and then the layer list in fp16, one layer at a time, over every batch; see(name, t, c_real) is
        called with each named tensor t (fp16 NHWC, channels c_real .. zero padding)"""
        with torch.no_grad():
            for x in batches:
                x = x.contiguous()
                fmt, n, h, w = engine._input_format(x, self.input_channels)
                st = self.state_for(n, h, w, slot='calibrate')
                with torch.cuda.device(self.device):
                    engine.EnginePlan.run_backbone(self, x, fmt, st)
                    t = st.bufs[self.stage_in]
                    if t.shape[3] != self.qbuf_channels[0]:       # a 32-channel stem in front of stages padded to 64
                        t = F.pad(t, (0, self.qbuf_channels[0] - t.shape[3]))
                    see(STEM, t, self.stem_channels_real)
                    outs = {0: t}
                    for c in self.layers:
                        res = outs[c.res] if c.res is not None else None
                        if ops.conv2d_supported(c.cin, c.cout, c.ks, c.stride):
                            if c.w16 is None:
                                c.w16 = ops.pack_conv_weight(c.ref_w).to(self.device)
                            y = ops.conv2d_nhwc(outs[c.src].contiguous(), c.w16, c.ref_b, c.cin, c.cout, c.ks, c.stride, c.relu,
                                                residual=res)
                        else:
                            y = F.conv2d(outs[c.src].permute(0, 3, 1, 2).float(), c.ref_w.to(self.device), c.ref_b, stride=c.stride,
                                         padding=c.ks // 2).permute(0, 2, 3, 1)
                            if res is not None:
                                y = y + res.float()
                            if c.relu:
                                y = y.relu()
                            y = y.half().contiguous()
                        see(c.name, y, c.cout_real)
                        outs[c.dst] = y
            self._shape_cache = dict((k, v) for k, v in self._shape_cache.items() if k[3] != 'calibrate')

    def calibrate(self, batches):
        """batches: iterable of device frame batches (any format the stem accepts) -> {tensor name: amax (float)} over all of
        them (amax with torch).  Runs the stem launches and then the layer list in fp16, one layer at a time."""
        amax = dict((k, 0.0) for k in self.tensor_names)

        def see(name, t, c_real):
            amax[name] = max(amax[name], float(t.float().abs().max()))

        self._calibration_walk(batches, see)
        return amax

    def calibrate_histograms(self, batches):
        """the same fp16 walk -> {tensor name: numpy int64 [32768]}: the magnitude histogram (ops.abs_histogram_f16) of every
        named tensor's real channels over all batches, from which lfd_amd/calibration.py chooses the thresholds"""
        hists = {}

        def see(name, t, c_real):
            if name not in hists:
                hists[name] = torch.zeros(ops.ABS_HIST_BINS, dtype=torch.int64, device=self.device)
            ops.abs_histogram_f16(t.contiguous(), c_real, out=hists[name])

        self._calibration_walk(batches, see)
        zero = numpy.zeros(ops.ABS_HIST_BINS, dtype=numpy.int64)
        return dict((k, hists[k].cpu().numpy() if k in hists else zero.copy()) for k in self.tensor_names)

    def set_scales(self, amax):
        """{tensor name: amax} -> the constants of every launch; self.scales = {name: (amax, scale)}"""
        missing = [k for k in self.tensor_names if k not in amax]
        if missing:
            raise KeyError('calibration misses the tensors %s' % missing)
        dev = self.device
        self.scales = dict((k, (float(amax[k]), act_scale(float(amax[k])))) for k in self.tensor_names)
        self.inv_stem_scale = float(torch.tensor(1.0 / self.scales[STEM][1], dtype=torch.float64).float())
        for c in self.layers:
            c.s_in, c.s_out = self.scales[c.src_name][1], self.scales[c.name][1]
            c.s_res = self.scales[c.res_name][1] if c.res is not None else None
            mult, biasq, c.res_mult = epilogue_constants(c.s_in, c.s_w, c.ref_b, c.s_out, c.s_res)
            c.mult, c.biasq = mult.to(dev).contiguous(), biasq.to(dev).contiguous()

    # ---- shape-dependent state: the parent's (fp16 stem, tap and head buffers) plus the int8 maps
    def state_for(self, n, h, w, slot=0):
        st = super().state_for(n, h, w, slot)
        if not hasattr(st, 'qbufs'):
            st.qbufs = {}
            if self.stem_int8_formats and slot != 'calibrate':
                # the fp16 stem map (the largest tensor of the network) is only needed by a call in another frame format:
                # stem_f16() allocates it on first use
                del st.bufs[self.stage_in]
            with torch.cuda.device(self.device):
                for b, sc in self.qbuf_scale.items():
                    if b in self.unwritten:                   # the map between a fused block's convs stays on chip
                        continue
                    hh, ww, s = h, w, sc
                    while s > 1:
                        hh, ww = (hh + 1) // 2, (ww + 1) // 2
                        s //= 2
                    st.qbufs[b] = torch.zeros((n, hh, ww, self.qbuf_channels[b]), dtype=torch.int8, device=self.device)
        return st

    # ---- execution
    def stem_f16(self, st):
        """the fp16 stem map of this shape and slot (dropped by state_for under stem_int8: allocated on first use)"""
        if self.stage_in not in st.bufs:
            hh, ww = st.dims[self.stage_in]
            with torch.cuda.device(self.device):
                st.bufs[self.stage_in] = torch.empty((st.n, hh, ww, self.buf_channels[self.stage_in]), dtype=torch.float16,
                                                     device=self.device)
        return st.bufs[self.stage_in]

    def run_stem(self, x, fmt, st):
        """fmt in stem_int8_formats: the stem launch writes int8 buffer 0 itself (lfd_stem_conv_i8 / lfd_stem_faster_fused_i8
        with inv_stem_scale), nothing else.  Otherwise the parent's stem launches into the fp16 buffer, then the quantise launch
        (unless the first 'entry' launch of the 'full' route reads the fp16 map itself).  -> whether the stem wrote int8 buffer 0
        itself; run_backbone hands that to run_stages.  self.front and st.front are a log of what was launched, nothing reads them
        to decide a launch: {'stem': entry point, 'quantise': whether the quantise launch ran, 'entry_in_format': in_format of
        the first 'entry' launch behind the stem under 'full' (filled by run_stages), else None}.  They are written when Python
        runs these methods -- eagerly and while a graph is captured -- and NOT by a graph replay: after a replay they still show
        the last eager or captured call."""
        st.front = self.front = dict(stem=None, quantise=False, entry_in_format=None)
        if fmt in self.stem_int8_formats:
            l, sp = lib(), stream_ptr()
            if self.stem_fused is not None:
                c0, w1, b1, w2, b2, w3, b3, w4, b4, _dst = self.stem_fused
                st.front['stem'] = 'lfd_stem_faster_fused_i8'
                check(l.lfd_stem_faster_fused_i8(ptr(x), fmt, st.n, st.h, st.w, c0, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3),
                                                 ptr(b3), ptr(w4), ptr(b4), self.inv_stem_scale, ptr(st.qbufs[0]), sp),
                      'lfd_stem_faster_fused_i8')
            else:
                c0, w1, b1, w2, b2 = self.stem_first
                st.front['stem'] = 'lfd_stem_conv_i8'
                check(l.lfd_stem_conv_i8(ptr(x), fmt, st.n, st.h, st.w, c0, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                         self.inv_stem_scale, ptr(st.qbufs[0]), sp), 'lfd_stem_conv_i8')
            return True
        st.front['stem'] = 'fp16'
        self.stem_f16(st)
        engine.EnginePlan.run_backbone(self, x, fmt, st)
        if self.entry_f16 is None:
            st.front['quantise'] = True
            self.run_quantise(st)
        return False

    def run_quantise(self, st):
        src = self.stem_f16(st)
        l, sp = lib(), stream_ptr()
        if src.shape[3] == self.qbuf_channels[0]:
            check(l.lfd_quantize_nhwc_f16_i8(ptr(src), ptr(st.qbufs[0]), src.numel(), self.inv_stem_scale, sp),
                  'lfd_quantize_nhwc_f16_i8')
        else:
            check(l.lfd_quantize_pad_nhwc_f16_i8(ptr(src), ptr(st.qbufs[0]), src.numel() // src.shape[3], src.shape[3],
                                                 self.qbuf_channels[0], self.inv_stem_scale, sp), 'lfd_quantize_pad_nhwc_f16_i8')

    def run_layer(self, c, st):
        src = st.qbufs[c.src]
        d = _lib.ConvDesc(st.n, src.shape[1], src.shape[2], c.cin, c.cout, c.ks, c.stride, int(c.relu), 0, 0)
        check(lib().lfd_conv2d_nhwc_i8(C.byref(d), ptr(src), ptr(c.w), ptr(c.mult), ptr(c.biasq),
                                       ptr(st.qbufs[c.res]) if c.res is not None else None, c.res_mult, ptr(st.qbufs[c.dst]),
                                       ptr(st.bufs[c.tap]) if c.tap is not None else None, c.s_out, stream_ptr()),
              'lfd_conv2d_nhwc_i8')

    def run_pair(self, d, c, st):
        """d: the 1x1 stride-2 identity branch, c: the 3x3 stride-2 conv of the same input, one launch"""
        src = st.qbufs[c.src]
        check(lib().lfd_conv2d_downsample_nhwc_i8(st.n, src.shape[1], src.shape[2], c.cin, c.cout, ptr(src), ptr(c.w), ptr(c.mult),
                                                  ptr(c.biasq), ptr(d.w), ptr(d.mult), ptr(d.biasq), ptr(st.qbufs[c.dst]),
                                                  ptr(st.qbufs[d.dst]), stream_ptr()), 'lfd_conv2d_downsample_nhwc_i8')

    def run_block(self, c1, c2, st):
        """a whole residual block (c1 -> c2 + the block's input) in one launch, the tap on it if the block is one"""
        src = st.qbufs[c1.src]
        check(lib().lfd_block_i8_fused(st.n, src.shape[1], src.shape[2], ptr(src), ptr(c1.w), ptr(c1.mult), ptr(c1.biasq),
                                       ptr(c2.w), ptr(c2.mult), ptr(c2.biasq), c2.res_mult, ptr(st.qbufs[c2.dst]),
                                       ptr(st.bufs[c2.tap]) if c2.tap is not None else None, c2.s_out, stream_ptr()),
              'lfd_block_i8_fused')

    def run_block128(self, c1, c2, st):
        """a whole 128-channel residual block (c1 -> c2 + the block's input) in one launch, the tap on it if the block is one"""
        src = st.qbufs[c1.src]
        check(lib().lfd_block128_i8_fused(st.n, src.shape[1], src.shape[2], ptr(src), ptr(c1.w), ptr(c1.mult), ptr(c1.biasq),
                                          ptr(c2.w), ptr(c2.mult), ptr(c2.biasq), c2.res_mult, ptr(st.qbufs[c2.dst]),
                                          ptr(st.bufs[c2.tap]) if c2.tap is not None else None, c2.s_out, stream_ptr()),
              'lfd_block128_i8_fused')

    def run_entry(self, d, c1, c2, st, f16):
        """a whole 64-channel stage-entry block (d: the identity branch, c1, c2 adding d) in one launch; f16: the input is the
        fp16 stem map, quantised on the way in"""
        src = self.stem_f16(st) if f16 else st.qbufs[c1.src]
        check(lib().lfd_entry_i8_fused(st.n, src.shape[1], src.shape[2], 1 if f16 else 0, src.shape[3], ptr(src),
                                       self.inv_stem_scale if f16 else 0.0, ptr(c1.w), ptr(c1.mult), ptr(c1.biasq), ptr(d.w),
                                       ptr(d.mult), ptr(d.biasq), ptr(c2.w), ptr(c2.mult), ptr(c2.biasq), c2.res_mult,
                                       ptr(st.qbufs[c2.dst]), stream_ptr()), 'lfd_entry_i8_fused')

    def run_stages(self, st, after=None, stem_i8=False):
        """the int8 launches of the stages.  stem_i8: the stem launch wrote int8 buffer 0 itself (run_stem's return value), so
        the first 'entry' launch of the 'full' route reads it instead of the fp16 stem map"""
        base = len(self.convs)
        if self.fused:
            for k, la in enumerate(self.launches):
                if after and base + k in after:
                    after[base + k]()
                cs = [self.layers[i] for i in la.layers]
                if la.kind == 'pair':
                    self.run_pair(cs[0], cs[1], st)
                elif la.kind == 'block':
                    self.run_block(cs[0], cs[1], st)
                elif la.kind == 'block128':
                    self.run_block128(cs[0], cs[1], st)
                elif la.kind == 'entry':
                    f16 = k == self.entry_f16 and not stem_i8
                    if cs[0].src == 0 and getattr(st, 'front', None) is not None:
                        st.front['entry_in_format'] = 1 if f16 else 0
                    self.run_entry(cs[0], cs[1], cs[2], st, f16)
                else:
                    self.run_layer(cs[0], st)
            if after and base + len(self.launches) in after:
                after[base + len(self.launches)]()
            return
        for li, c in enumerate(self.layers):
            if after and base + li in after:
                after[base + li]()
            self.run_layer(c, st)
        if after and base + len(self.layers) in after:
            after[base + len(self.layers)]()

    def run_backbone(self, x, fmt, st, after=None):
        if self.scales is None:
            raise RuntimeError('Int8Plan: no scales yet (calibrate() + set_scales(), or deployment.build_int8_engine)')
        stem_i8 = self.run_stem(x, fmt, st)
        self.run_stages(st, after, stem_i8=stem_i8)
