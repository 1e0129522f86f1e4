"""The INT8 deployment mode (lfd_amd.deployment, csrc/conv_i8.hip, csrc/block_i8.hip, csrc/entry_i8.hip, csrc/block128_i8.hip; csrc/i8_impl.h), its
'full' route with and without the block128 and stem_int8 options, its fused route and its default layer-by-layer route, against the 'fp16' mode, frames resident in device memory (NHWC fp16,
1920 x 1080 unless --size=HxW):

    python tools/bench_int8.py [CONFIG ...] [--bs=8,1] [--size=1080x1920] [--out=FILE] [--only=SECTION,...]

per configuration (default WIDERFACE_LFD_S, WIDERFACE_LFD_XS, TT100K_LFD_L, TL_LFD_L, WIDERFACE_LFD_L) and batch size (--only: the
sections to run, default all of them):
  * stages: the quantise launch (where the route has one) + the int8 plan's stage launches (Int8Plan.run_stages), full + block128
    + stem_int8 (build_int8_engine(..., fused='full', block128=True, stem_int8=True): no quantise launch, the first entry launch
    reads int8), full + block128, full (fused='full'), fused (fused=True) and layer by layer, against the fp16 plan's stage launches
    (EnginePlan._run_convs: fused blocks, downsample pairs), eager launches on one stream;
  * forward: Int8Engine.forward_resident of the five int8 sides against LFD.forward_resident in the 'fp16' mode, each as one graph
    replay;
  * detect: forward + LFD.detect (decode, threshold, NMS on the device) behind each of the six forwards;
  * stem: the stem launch alone on NHWC fp16 and on NHWC uint8 frames (configurations with an int8 stem): the int8-output call
    (lfd_stem_conv_i8 / lfd_stem_faster_fused_i8) against the fp16-output call plus what follows it today -- the quantise launch
    under fused=True, and under 'full' the difference between the first entry launch's fp16-in and int8-in times;
  * layers: every distinct int8 launch of the layer-by-layer plan at that frame size on its own -- microseconds per call and
    TOP/s (2 * n * oh * ow * cout * cin * ks^2 integer operations of the padded layer over the call time);
  * fused_launches: every distinct lfd_block_i8_fused / lfd_conv2d_downsample_nhwc_i8 launch of the fused plan next to the two
    layer-by-layer launches it replaces (their call times added), same units;
  * entry_launches: every distinct lfd_entry_i8_fused launch of the full plan in the int8 input format next to the pair + conv
    launches of the fused route it replaces, and the one behind the stem also in the fp16 input format next to quantise + pair
    + conv;
  * block128_launches: every distinct lfd_block128_i8_fused launch of the full + block128 plan next to the two lfd_conv2d_nhwc_i8
    launches it replaces, each with and without the fp16 tap, same protocol and units.
The sides follow tools/bench_resnet.py: HIP events around `reps` back-to-back calls, alternating the sides, the median of
`rounds` such windows divided by `reps` and max - min of the windows as the spread -- call times (kernel + launch), not profiler
kernel times.  The calibration set is four seeded frames of a quarter of the size: scales do not change a launch's time.

Records, no pass / fail gate.  Prints one JSON line; --out=FILE also keeps the results gathered so far after every measurement."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lfd_amd import INT8Calibrator, build_int8_engine, configs, engine, ops  # noqa: E402


def opt(name, default):
    return ([a[len(name) + 3:] for a in sys.argv[1:] if a.startswith('--%s=' % name)] or [default])[0]


NAMES = [a for a in sys.argv[1:] if not a.startswith('--')] or ['WIDERFACE_LFD_S', 'WIDERFACE_LFD_XS', 'TT100K_LFD_L', 'TL_LFD_L',
                                                               'WIDERFACE_LFD_L']
SECTIONS = ('stages', 'forward', 'detect', 'stem', 'layers', 'fused_launches', 'entry_launches', 'block128_launches')
ONLY = opt('only', ','.join(SECTIONS)).split(',')
assert all(s_ in SECTIONS for s_ in ONLY), 'sections: %s' % ', '.join(SECTIONS)
BATCHES = [int(v) for v in opt('bs', '8,1').split(',')]
H, W = [int(v) for v in opt('size', '1080x1920').split('x')]
OUT = opt('out', None)
REPS, ROUNDS = 20, 7
assert torch.cuda.is_available(), 'bench_int8.py measures on the GPU'
res = dict(workload='INT8 deployment mode vs the fp16 mode, %dx%d NHWC fp16 frames' % (W, H), reps=REPS, rounds=ROUNDS, configs={})


def save():
    if OUT:
        json.dump(res, open(OUT, 'w'), indent=1)


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def pair(*sides, reps=REPS):
    """-> [(median ms, max - min ms)] per side over alternating windows"""
    for _ in range(2):
        for f in sides:
            window_ms(f, reps)
    ts = [[] for _ in sides]
    for _ in range(ROUNDS):
        for k, f in enumerate(sides):
            ts[k].append(window_ms(f, reps))
    return [(float(np.median(t)), float(max(t) - min(t))) for t in ts]


def sides(nd=4, **fns):
    """pair() over the named sides (int8_full, int8_fused, int8 = layer by layer, fp16, int8_full_b128, int8_full_b128_stem) ->
    their medians, spreads and ratios"""
    reps = fns.pop('reps', REPS)
    assert sorted(fns) == sorted(('int8_full', 'int8_fused', 'int8', 'fp16', 'int8_full_b128', 'int8_full_b128_stem'))
    tags = list(fns)
    got = dict(zip(tags, pair(*[fns[k] for k in tags], reps=reps)))
    out = {}
    for tag in tags:
        out[tag] = round(got[tag][0], nd)
        out[tag + '_spread'] = round(got[tag][1], nd)
    got = [got[k] for k in ('int8_full', 'int8_fused', 'int8', 'fp16', 'int8_full_b128', 'int8_full_b128_stem')]
    out['int8_full_over_fp16'] = round(got[0][0] / got[3][0], 3)
    out['int8_fused_over_fp16'] = round(got[1][0] / got[3][0], 3)
    out['int8_over_fp16'] = round(got[2][0] / got[3][0], 3)
    out['int8_fused_over_int8'] = round(got[1][0] / got[2][0], 3)
    out['int8_full_over_fused'] = round(got[0][0] / got[1][0], 3)
    out['int8_full_b128_over_fp16'] = round(got[4][0] / got[3][0], 3)
    out['int8_full_b128_over_full'] = round(got[4][0] / got[0][0], 3)
    # does full + block128 differ from full by more than both spreads?
    out['b128_differs_from_full'] = bool(abs(got[4][0] - got[0][0]) > max(got[4][1], got[0][1]))
    out['int8_full_b128_stem_over_fp16'] = round(got[5][0] / got[3][0], 3)
    out['int8_full_b128_stem_over_full_b128'] = round(got[5][0] / got[4][0], 3)
    # does the stem_int8 side differ from full + block128, and from fp16, by more than both spreads?
    out['stem_differs_from_full_b128'] = bool(abs(got[5][0] - got[4][0]) > max(got[5][1], got[4][1]))
    out['stem_differs_from_fp16'] = bool(abs(got[5][0] - got[3][0]) > max(got[5][1], got[3][1]))
    return out


with torch.no_grad():
    for name in NAMES:
        m = configs.build_model(name)
        configs.perturb_weights(m)
        m.eval().cuda()
        frames = (torch.rand(4, 3, H // 4, W // 4, generator=torch.Generator().manual_seed(5)) * 2 - 1).numpy()
        cache = os.path.join(tempfile.mkdtemp(prefix='bench_int8_'), 'cal.json')
        eng = build_int8_engine(m, INT8Calibrator(frames, cache, batch_size=2))
        engf = build_int8_engine(m, INT8Calibrator(frames, cache, batch_size=2), fused=True)      # from the cache just written
        engF = build_int8_engine(m, INT8Calibrator(frames, cache, batch_size=2), fused='full')
        engB = build_int8_engine(m, INT8Calibrator(frames, cache, batch_size=2), fused='full', block128=True)
        engS = build_int8_engine(m, INT8Calibrator(frames, cache, batch_size=2), fused='full', block128=True, stem_int8=True)
        assert not engf.calibrated and not engF.calibrated and not engB.calibrated and not engS.calibrated
        plan8, planf, planF, planB, planS = eng.plan, engf.plan, engF.plan, engB.plan, engS.plan
        plan16 = engine.get_plan(m, m._backbone, m._neck, m._head, torch.device('cuda', torch.cuda.current_device()))
        ent = res['configs'][name] = dict(int8_launches=len(plan8.layers) + 1, int8_fused_launches=planf.int8_launches() + 1,
                                        int8_full_launches=planF.int8_launches() + (planF.entry_f16 is None),
                                        int8_full_b128_launches=planB.int8_launches() + (planB.entry_f16 is None),
                                        int8_full_b128_stem_launches=planS.int8_launches() + (planS.entry_f16 is None
                                                                                               and 1 not in planS.stem_int8_formats),
                                        stem_int8_formats=sorted(planS.stem_int8_formats),
                                        fp16_stage_launches=len(plan16.convs))
        for bs in BATCHES:
            x = (torch.rand(bs, H, W, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1).half()
            meta = torch.tensor([[float(W), float(H), 1.0]] * bs, device='cuda')
            fmt = engine.IN_NHWC_F16
            st8, stf, st16 = plan8.state_for(bs, H, W), planf.state_for(bs, H, W), plan16.state_for(bs, H, W)
            stF, stB, stS = planF.state_for(bs, H, W), planB.state_for(bs, H, W), planS.state_for(bs, H, W)
            plan8.run_all(x, fmt, st8)
            planf.run_all(x, fmt, stf)
            planF.run_all(x, fmt, stF)
            planB.run_all(x, fmt, stB)
            planS.run_all(x, fmt, stS)
            plan16.run_all(x, fmt, st16)
            torch.cuda.synchronize()
            r = ent['bs%d' % bs] = {}

            def stages8():
                plan8.run_quantise(st8)
                plan8.run_stages(st8)

            def stagesf():
                planf.run_quantise(stf)
                planf.run_stages(stf)

            def stagesF():
                if planF.entry_f16 is None:
                    planF.run_quantise(stF)
                planF.run_stages(stF)

            def stagesB():
                if planB.entry_f16 is None:
                    planB.run_quantise(stB)
                planB.run_stages(stB)

            stem_i8 = fmt in planS.stem_int8_formats

            def stagesS():                                     # behind an int8 stem: no quantise launch, the entry launch reads int8
                if not stem_i8 and planS.entry_f16 is None:
                    planS.run_quantise(stS)
                planS.run_stages(stS, stem_i8=stem_i8)

            assert torch.equal(stB.cls, st8.cls) and torch.equal(stB.reg, st8.reg), 'block128 must equal the default bit for bit'
            assert torch.equal(stS.cls, st8.cls) and torch.equal(stS.reg, st8.reg), 'stem_int8 must equal the default bit for bit'
            assert torch.equal(stf.cls, st8.cls) and torch.equal(stf.reg, st8.reg), 'the fused route must equal the default bit for bit'
            assert torch.equal(stF.cls, st8.cls) and torch.equal(stF.reg, st8.reg), 'the full route must equal the default bit for bit'
            if 'stages' in ONLY:
                r['stages_ms'] = sides(int8_full=stagesF, int8_fused=stagesf, int8=stages8, fp16=lambda: plan16._run_convs(st16),
                                       int8_full_b128=stagesB, int8_full_b128_stem=stagesS, reps=5)
                save()
            eng.use_graph = engf.use_graph = engF.use_graph = engB.use_graph = engS.use_graph = m.use_graph = True
            if 'forward' in ONLY:
                r['forward_ms'] = sides(int8_full=lambda: engF.forward_resident(x), int8_fused=lambda: engf.forward_resident(x),
                                        int8=lambda: eng.forward_resident(x), fp16=lambda: m.forward_resident(x),
                                        int8_full_b128=lambda: engB.forward_resident(x),
                                        int8_full_b128_stem=lambda: engS.forward_resident(x))
                save()
            if 'detect' in ONLY:
                thr = float(np.quantile(st16.cls.sigmoid().float().cpu().numpy(), 0.999)) if st16.cls.shape[2] == 1 else 0.5
                r['detect_ms'] = sides(int8_full=lambda: engF.detect(x, meta, score_thr=thr),
                                       int8_fused=lambda: engf.detect(x, meta, score_thr=thr),
                                       int8=lambda: eng.detect(x, meta, score_thr=thr),
                                       fp16=lambda: m.detect(m.forward_resident(x), meta, score_thr=thr),
                                       int8_full_b128=lambda: engB.detect(x, meta, score_thr=thr),
                                       int8_full_b128_stem=lambda: engS.detect(x, meta, score_thr=thr))
                save()
            eng.use_graph = engf.use_graph = engF.use_graph = engB.use_graph = engS.use_graph = m.use_graph = False
            # ---- the stem launch alone: int8 output against fp16 output plus what follows it today
            if 'stem' in ONLY and planS.stem_int8_formats and planF.entry_f16 is not None:
                cd, c1, c2 = [planf.layers[i] for i in planF.launches[planF.entry_f16].layers]
                sl = {}
                for tag, xf, f in (('fp16', x, engine.IN_NHWC_F16),
                                   ('uint8', torch.randint(0, 256, (bs, H, W, 3), dtype=torch.uint8, device='cuda'), engine.IN_NHWC_U8)):
                    if f not in planS.stem_int8_formats:
                        continue

                    def stem_f16_quantise():
                        engine.EnginePlan.run_backbone(planf, xf, f, stf)
                        planf.run_quantise(stf)

                    (ti, si), (th, sh), (tq, sq), (te, se), (t8, s8) = pair(
                        lambda: planS.run_stem(xf, f, stS), lambda: engine.EnginePlan.run_backbone(planf, xf, f, stf), stem_f16_quantise,
                        lambda: planf.run_entry(cd, c1, c2, stf, True), lambda: planf.run_entry(cd, c1, c2, stf, False))
                    today_full = th + te - t8
                    sl[tag] = dict(map='%dx%d' % tuple(stS.qbufs[0].shape[1:3]), stem_i8_us=round(1e3 * ti, 2),
                                   stem_i8_spread_us=round(1e3 * si, 2), stem_f16_us=round(1e3 * th, 2),
                                   stem_f16_spread_us=round(1e3 * sh, 2), stem_f16_quantise_us=round(1e3 * tq, 2),
                                   stem_f16_quantise_spread_us=round(1e3 * sq, 2), entry_f16_us=round(1e3 * te, 2),
                                   entry_f16_spread_us=round(1e3 * se, 2), entry_i8_us=round(1e3 * t8, 2),
                                   entry_i8_spread_us=round(1e3 * s8, 2), stem_f16_plus_entry_difference_us=round(1e3 * today_full, 2),
                                   i8_over_f16_quantise=round(ti / tq, 3), i8_over_f16_plus_entry_difference=round(ti / today_full, 3),
                                   i8_over_f16=round(ti / th, 3))
                r['stem'] = sl
                save()
                planS.run_all(x, fmt, stS)                       # leave the fp16 frame's maps behind for the sections below
                planf.run_all(x, fmt, stf)
            # ---- every distinct int8 launch on its own
            layers = {}

            def layer_key(c):
                src = st8.qbufs[c.src]
                return '%dto%d k%d s%d %dx%d%s%s' % (c.cin, c.cout, c.ks, c.stride, src.shape[1], src.shape[2],
                                                      ' +res' if c.res is not None else '', ' +tap' if c.tap is not None else '')

            def layer_ops(c):
                return 2.0 * st8.qbufs[c.dst].numel() * c.cin * c.ks * c.ks

            if 'layers' in ONLY:
                for c in plan8.layers:
                    key = layer_key(c)
                    if key in layers:
                        continue
                    (t, spread), = pair(lambda: plan8.run_layer(c, st8))
                    layers[key] = dict(us=round(1e3 * t, 2), spread_us=round(1e3 * spread, 2),
                                       TOPs=round(layer_ops(c) / (t * 1e-3) / 1e12, 1))
                r['layers'] = layers
                save()
            # ---- every distinct fused launch against the two layer-by-layer launches it replaces
            fl = {}
            if 'fused_launches' in ONLY:
                for la in planf.launches:
                    if la.kind == 'conv':
                        continue
                    ca, cb = [planf.layers[i] for i in la.layers]
                    pa, pb = [plan8.layers[i] for i in la.layers]
                    key = '%s: %s | %s' % (la.kind, layer_key(pa), layer_key(pb))
                    if key in fl:
                        continue
                    run = (lambda: planf.run_pair(ca, cb, stf)) if la.kind == 'pair' else (lambda: planf.run_block(ca, cb, stf))

                    def two():
                        plan8.run_layer(pa, st8)
                        plan8.run_layer(pb, st8)

                    (tf, sf), (t2, s2) = pair(run, two)
                    ops_ = layer_ops(pa) + layer_ops(pb)
                    fl[key] = dict(fused_us=round(1e3 * tf, 2), fused_spread_us=round(1e3 * sf, 2), two_launches_us=round(1e3 * t2, 2),
                                   two_launches_spread_us=round(1e3 * s2, 2), fused_TOPs=round(ops_ / (tf * 1e-3) / 1e12, 1),
                                   fused_over_two=round(tf / t2, 3))
                r['fused_launches'] = fl
                save()
            # ---- every distinct entry launch against the launches of the fused route it replaces (the fused plan's buffers)
            el = {}
            if 'entry_launches' in ONLY:
                for k, la in enumerate(planF.launches):
                    if la.kind != 'entry':
                        continue
                    cd, c1, c2 = [planf.layers[i] for i in la.layers]
                    key = 'entry: %s | %s' % (layer_key(c1), layer_key(c2))
                    if key in el and k != planF.entry_f16:
                        continue

                    def pair_conv():
                        planf.run_pair(cd, c1, stf)
                        planf.run_layer(c2, stf)

                    def quantise_pair_conv():
                        planf.run_quantise(stf)
                        pair_conv()

                    ops_ = layer_ops(cd) + layer_ops(c1) + layer_ops(c2)
                    (te, se), (tp, sp_) = pair(lambda: planf.run_entry(cd, c1, c2, stf, False), pair_conv)
                    e = el[key] = dict(entry_us=round(1e3 * te, 2), entry_spread_us=round(1e3 * se, 2), pair_conv_us=round(1e3 * tp, 2),
                                       pair_conv_spread_us=round(1e3 * sp_, 2), entry_TOPs=round(ops_ / (te * 1e-3) / 1e12, 1),
                                       entry_over_pair_conv=round(te / tp, 3))
                    if k == planF.entry_f16:
                        (te, se), (tq, sq) = pair(lambda: planf.run_entry(cd, c1, c2, stf, True), quantise_pair_conv)
                        e.update(entry_f16_us=round(1e3 * te, 2), entry_f16_spread_us=round(1e3 * se, 2),
                                 quantise_pair_conv_us=round(1e3 * tq, 2), quantise_pair_conv_spread_us=round(1e3 * sq, 2),
                                 entry_f16_over_quantise_pair_conv=round(te / tq, 3))
                r['entry_launches'] = el
                save()
            # ---- every distinct block128 launch against the two lfd_conv2d_nhwc_i8 launches it replaces, with and without the tap
            bl = {}
            if 'block128_launches' in ONLY:
                for la in planB.launches:
                    if la.kind != 'block128':
                        continue
                    c1, c2 = [plan8.layers[i] for i in la.layers]
                    src, mid, dst = st8.qbufs[c1.src], st8.qbufs[c1.dst], st8.qbufs[c2.dst]
                    shape_key = 'block128: %dx%d' % (src.shape[1], src.shape[2])
                    if shape_key + ' +tap' in bl:
                        continue
                    tapbuf = st8.bufs[c2.tap] if c2.tap is not None else torch.empty(dst.shape, dtype=torch.float16, device='cuda')
                    ops_ = layer_ops(c1) + layer_ops(c2)
                    for tap in (True, False):
                        sc, tb = (c2.s_out, tapbuf) if tap else (None, None)

                        def one():
                            ops.block128_i8_fused(src, c1.w, c1.mult, c1.biasq, c2.w, c2.mult, c2.biasq, c2.res_mult, out_scale=sc,
                                                  out=dst, out_f16=tb)

                        def two():
                            ops.conv2d_nhwc_i8(src, c1.w, c1.mult, c1.biasq, 128, 3, 1, True, out=mid)
                            ops.conv2d_nhwc_i8(mid, c2.w, c2.mult, c2.biasq, 128, 3, 1, True, residual=src, res_mult=c2.res_mult,
                                               out_scale=sc, out=dst, out_f16=tb)

                        (tf, sf), (t2, s2) = pair(one, two)
                        bl[shape_key + (' +tap' if tap else '')] = dict(
                            block128_us=round(1e3 * tf, 2), block128_spread_us=round(1e3 * sf, 2), two_launches_us=round(1e3 * t2, 2),
                            two_launches_spread_us=round(1e3 * s2, 2), block128_TOPs=round(ops_ / (tf * 1e-3) / 1e12, 1),
                            block128_over_two=round(tf / t2, 3), in_plan=(c2.tap is not None) == tap)
                r['block128_launches'] = bl
                save()
            del x, st8, stf, stF, stB, stS, st16
            plan8._shape_cache.clear()
            planf._shape_cache.clear()
            planF._shape_cache.clear()
            planB._shape_cache.clear()
            planS._shape_cache.clear()
            plan16._shape_cache.clear()
            m.__dict__.get('_step_graphs', {}).clear()
            torch.cuda.empty_cache()
        del m, eng, engf, engF, engB, engS, plan8, planf, planF, planB, planS, plan16
        torch.cuda.empty_cache()
print(json.dumps(res))
