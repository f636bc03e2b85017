"""-m gpu: the epilogues of conv_c8_kernel where they read their arguments and choose their paths.

The epilogues read their arguments once per tile into held registers, dispatch once per tile to a body specialised for the
epilogue kind and the layout of the fp32 tensors, and address every tensor as a wave-uniform base plus a lane offset.  What
can go wrong with that is placement, not arithmetic, so the checks are exact:

  * every problem runs alone, as the first problem of dkt_conv2d_c8_pair and as the second problem beside a problem of another
    shape, kind and channel count -- all outputs bit for bit equal (cached arguments taken from the wrong problem);
  * a batch with more tiles than resident blocks against the same problem one batch item at a time (per-tile values that are
    not refreshed when a block walks on to its next tile).

Both also run against fp64 (_c8_ref.py) with the bounds test_gpu_c8_scaled.py uses: CONV 3e-6, GRU 4e-6, HEAD 2e-5 relative to
the output maximum.  No bound is new.

Shapes (B, H, W) = (1, 33, 37) and (2, 46, 78) are ragged in rows and columns for every tile shape; Cout 126 + 2 tail channels
and Cout 20 leave padded channels (and, in the 128- and 256-channel tile shapes, idle waves); out_c8_ch0 = 64 writes behind
another layer's channels; the gates run with NCHW and with C4 fp32 tensors."""
import pytest
import torch

import _c8_ref as R
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

CONV, GRU, HEAD = 3e-6, 4e-6, 2e-5
SHAPES = [(1, 33, 37), (2, 46, 78)]


def _c8():
    from dkt_stereo_amd import conv_c8
    return conv_c8


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, device=DEV, generator=g) * scale


def _acts(B, H, W, chans, g, kinds=None):
    xs = [R.operand((B, c, H, W), 1.0, 0, (kinds or ["randn"] * len(chans))[i], device=DEV, gen=g) for i, c in enumerate(chans)]
    return [R.pack_ref(x, s) for x, s in xs]


def _prefilled(B, C, H, W, scale, tail=0):
    """A destination whose interior already holds finite bytes in every channel: what a launch leaves alone stays comparable."""
    a = _c8().ActC8(B, C, H, W, DEV, scale=scale, tail=tail)
    ch = R.to_channels(a.t).clone()
    ch[:, :, :, 1:H + 1, 1:W + 1] = 0.25
    a.t = R.from_channels(ch)
    return a


def _item(a, i):
    """Batch item i of an ActC8 as an ActC8 of its own (a view)."""
    v = _c8().ActC8(1, a.C, a.H, a.W, DEV, scale=a.scale, tail=a.tail)
    v.tail_scale = a.tail_scale
    v.t = a.t[i:i + 1]
    return v


class _Problem:
    """One launch: make(b) -> (descriptor, outputs) with freshly allocated outputs (b: None = the whole batch, else one
    item); check(outputs) compares with fp64."""

    def __init__(self, kind, B, H, W, seed, cout=None, tail=0, ch0=0, c4=False, relu=True):
        c8 = _c8()
        self.kind, self.B, self.H, self.W, self.c4, self.relu, self.tail, self.ch0 = kind, B, H, W, c4, relu, tail, ch0
        torch.manual_seed(seed)
        g = _gen(seed)
        lay = lambda cin, co: torch.nn.Conv2d(cin, co, 3, padding=1).to(DEV)
        if kind == 0:
            self.acts = _acts(B, H, W, [48], g)
            self.layer = lay(48, cout)
            self.flow = _randn((B, tail, H, W), g, 3.0) if tail else None
            self.cd = ch0 + cout + tail
        elif kind == 4:
            self.acts = _acts(B, H, W, [48], g)
            self.layer = lay(48, cout)
            self.res = _randn((B, cout, H, W), g)
        elif kind in (1, 2):
            from dkt_stereo_amd.update import ConvGRU
            self.gru = ConvGRU(128, 64).to(DEV)
            self.h = torch.tanh(_randn((B, 128, H, W), g))
            self.acts = [R.pack_ref(self.h, R.calibrated_scale(self.h))] + _acts(B, H, W, [64], g, ["relu"])
            self.cz, self.cr, self.cq = (_randn((B, 128, H, W), g) for _ in range(3))
            self.z = torch.sigmoid(_randn((B, 128, H, W), g))
            self.zr = self.gru._merged_zr()
        else:
            from dkt_stereo_amd.update import FlowHead, _leading_outputs
            self.fh = FlowHead(128, 256, 2).to(DEV)
            self.acts = [R.pack_ref(*R.operand((B, 128, H, W), 1.0, 0, "tanh", device=DEV, gen=g))]
            self.conv2 = _leading_outputs(self.fh.conv2, 1)
        self.c8 = c8

    def _f(self, t, b):          # an fp32 epilogue operand in the launch's layout
        t = t if b is None else t[b:b + 1]
        return self.c8.to_c4(t) if self.c4 else t.contiguous()

    def _back(self, t, C):       # an fp32 output as NCHW
        return self.c8.from_c4(t, C) if self.c4 else t

    def make(self, b=None, cfg=0):
        c8 = self.c8
        B = self.B if b is None else 1
        H, W = self.H, self.W
        srcs = self.acts if b is None else [_item(a, b) for a in self.acts]
        new = lambda C: torch.full((B, C, H, W), 7.0, device=DEV)
        if self.kind == 0:
            cout = int(self.layer.weight.shape[0])
            out, oc = self._f(new(cout), None), _prefilled(B, self.cd, H, W, 64.0, tail=self.tail)
            flow = None if self.flow is None else (self.flow if b is None else self.flow[b:b + 1])
            d = c8.desc(srcs, self.layer, relu=self.relu, out=out, out_c8=oc, out_c8_ch0=self.ch0, tail=flow, f32_c4=self.c4)
            return d, [out, oc.t], oc
        if self.kind == 4:
            cout = int(self.layer.weight.shape[0])
            out, oc = self._f(new(cout), None), _prefilled(B, cout, H, W, 16.0)
            d = c8.desc(srcs, self.layer, relu=self.relu, out=out, out_c8=oc, epilogue=4, e0=self._f(self.res, b), f32_c4=self.c4)
            return d, [out, oc.t], oc
        if self.kind == 1:
            z, rh, rh8 = self._f(new(128), None), self._f(new(128), None), _prefilled(B, 128, H, W, srcs[0].scale)
            d = c8.desc(srcs, self.zr, out=z, epilogue=1, e0=self._f(self.cz, b), e1=self._f(self.cr, b), h=self._f(self.h, b),
                        out2=rh, out2_c8=rh8, f32_c4=self.c4)
            return d, [z, rh, rh8.t], rh8
        if self.kind == 2:
            out, oc = self._f(new(128), None), _prefilled(B, 128, H, W, srcs[0].scale)
            d = c8.desc(srcs, self.gru.convq, out=out, out_c8=oc, epilogue=2, e0=self._f(self.cq, b), e1=self._f(self.z, b),
                        h=self._f(self.h, b), f32_c4=self.c4)
            return d, [out, oc.t], oc
        hw = c8._head_weights(self.conv2)
        n_co = c8._ffi.lib().dkt_conv2d_c8_head_blocks(256, cfg)
        planes = torch.full((B, n_co * 9, H, W), 7.0, device=DEV)
        d = c8.desc(srcs, self.fh.conv1, relu=True, epilogue=3, head_w=hw, head_out=planes)
        return d, [planes], n_co

    def check(self, outs, extra):
        x64 = [R.unpack_ref(a) for a in self.acts]
        if self.kind in (0, 4):
            want = R.conv_ref64(x64, self.layer.weight, self.layer.bias, relu=self.relu, residual=self.res if self.kind == 4 else None)
            cout = want.shape[1]
            assert _rel(self._back(outs[0], cout), want) <= CONV, _rel(self._back(outs[0], cout), want)
            assert _rel(R.unpack_ref(extra, cout, self.ch0), want) <= CONV
            if self.tail:
                got_tail = R.unpack_ref(extra, self.tail, self.ch0 + cout)
                assert _rel(got_tail, self.flow) <= 2.0 ** -20                    # (the split keeps 22 bits)
            # the channels in front of the written ones keep their bytes; channels that fill the last written group are zero
            now = R.to_channels(extra.t)[:, :, :, 1:self.H + 1, 1:self.W + 1].float()
            c1 = self.ch0 + (cout + self.tail + 7) // 8 * 8
            assert float((now[:, :self.ch0] - 0.25).abs().max() if self.ch0 else 0.0) == 0.0
            assert float(now[:, self.ch0 + cout + self.tail:c1].abs().max() if c1 > self.ch0 + cout + self.tail else 0.0) == 0.0
        elif self.kind == 1:
            want_z, want_rh = R.gate_zr_ref64(self.gru, self.h, x64[1:], self.cz, self.cr)
            assert _rel(self._back(outs[0], 128), want_z) <= CONV
            assert _rel(self._back(outs[1], 128), want_rh) <= CONV
            assert _rel(R.unpack_ref(extra), want_rh) <= CONV
        elif self.kind == 2:
            want = R.gate_out_ref64(self.gru, x64[0], x64[1:], self.cq, self.z, self.h)
            got = self._back(outs[0], 128)
            assert _rel(got, want) <= CONV
            assert torch.equal(extra.t, R.pack_ref(got.contiguous(), extra.scale).t)
        else:
            B, H, W = self.B, self.H, self.W
            want = R.flow_head_ref64(self.fh.conv1, self.conv2, x64)
            planes = outs[0].double().view(B, extra, 9, H, W).sum(1)
            pad = torch.nn.functional.pad(planes, (1, 1, 1, 1))
            got = sum(pad[:, t, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)) + self.conv2.bias.double().view(1, 1, 1)
            e = float((got - want[:, 0]).abs().max()) / max(1.0, float(want.abs().max()))
            assert e <= HEAD, e


def _partner(residual, B):
    """The problem on the other side of a pair: another kind, shape and channel count."""
    if residual:
        return _Problem(4, 3 - B, 20, 45, seed=99, cout=40)
    return _Problem(0, 3 - B, 20, 45, seed=98, cout=20, relu=False)


def _three_ways(p, cfg):
    c8 = _c8()
    d, alone, extra = p.make(cfg=cfg)
    c8.launch(d, alone[0], cfg)
    p.check(alone, extra)
    q = _partner(p.kind == 0, p.B)
    dq, q_alone, _ = q.make(cfg=cfg)
    c8.launch(dq, q_alone[0], cfg)
    d0, first, _ = p.make(cfg=cfg)
    dq1, q_second, _ = q.make(cfg=cfg)
    c8.launch_pair(d0, dq1, first[0], cfg)
    dq0, q_first, _ = q.make(cfg=cfg)
    d1, second, _ = p.make(cfg=cfg)
    c8.launch_pair(dq0, d1, second[0], cfg)
    for name, got, want in (("first", first, alone), ("second", second, alone), ("partner second", q_second, q_alone),
                            ("partner first", q_first, q_alone)):
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), "%s of the pair: output %d differs from the launch alone (cfg %d)" % (name, i, cfg)


_K0 = {"c126_tail2": dict(cout=126, tail=2), "c20": dict(cout=20), "c64_ch0_64": dict(cout=64, ch0=64), "c20_norelu": dict(cout=20, relu=False)}


@torch.no_grad()
@pytest.mark.parametrize("cfg", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("variant", sorted(_K0))
def test_plain_epilogue_alone_and_in_both_places_of_a_pair(variant, shape, cfg):
    _three_ways(_Problem(0, *shape, seed=cfg + shape[1], **_K0[variant]), cfg)


@torch.no_grad()
@pytest.mark.parametrize("cfg", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kind,kw", [(0, dict(cout=126, tail=2)), (0, dict(cout=20)), (4, dict(cout=40))], ids=["c126_tail2", "c20", "residual_c40"])
def test_free_channel_counts_with_c4_tensors(kind, kw, shape, cfg):
    """Kinds 0 and 4 with [B][C/4][H][W][4] fp32 tensors: no product path launches them, the ABI accepts them -- the bodies
    that combine the clamped per-lane loads and the channel tests with 16-byte accesses."""
    _three_ways(_Problem(kind, *shape, seed=cfg + 5 * kind, c4=True, **kw), cfg)


@torch.no_grad()
@pytest.mark.parametrize("cfg", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("cout,relu", [(40, True), (64, False)])
def test_residual_epilogue_alone_and_in_both_places_of_a_pair(cout, relu, shape, cfg):
    _three_ways(_Problem(4, *shape, seed=cfg + cout, cout=cout, relu=relu), cfg)


@torch.no_grad()
@pytest.mark.parametrize("cfg", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("c4", [False, True], ids=["nchw", "c4"])
@pytest.mark.parametrize("kind", [1, 2])
def test_gate_epilogues_alone_and_in_both_places_of_a_pair(kind, c4, shape, cfg):
    _three_ways(_Problem(kind, *shape, seed=cfg + 10 * kind, c4=c4), cfg)


@torch.no_grad()
@pytest.mark.parametrize("cfg", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_head_epilogue_alone_and_in_both_places_of_a_pair(shape, cfg):
    _three_ways(_Problem(3, *shape, seed=cfg), cfg)


def _tiles(cfg, H, W, cout):
    rows, wm = {1: (8, 4), 2: (8, 2), 3: (8, 1), 4: (4, 1)}[cfg]
    n64 = (cout + 63) // 64
    return ((W + 31) // 32) * ((H + rows - 1) // rows) * ((n64 + wm - 1) // wm)


@torch.no_grad()
@pytest.mark.parametrize("kind,cfg,H,W,kw", [(1, 4, 46, 78, dict(c4=True)), (0, 2, 92, 156, dict(cout=126, tail=2)),
                                             (2, 3, 46, 78, dict()), (4, 4, 46, 78, dict(cout=40)), (3, 2, 46, 78, dict())],
                         ids=["zr-cfg4", "tail-cfg2", "q-cfg3", "residual-cfg4", "head-cfg2"])
def test_blocks_that_walk_several_tiles_equal_one_item_at_a_time(kind, cfg, H, W, kw):
    """More tiles than resident blocks (4-wave shapes hold two blocks per CU, 8-wave shapes one): every block walks on to a
    second tile, in another batch item."""
    c8 = _c8()
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    cout = {1: 256, 2: 128, 3: 256}.get(kind, kw.get("cout", 0))
    per_item = _tiles(cfg, H, W, cout)
    resident = cus * (1 if cfg <= 2 else 2)
    B = resident // per_item + 2
    assert B * per_item > resident
    p = _Problem(kind, B, H, W, seed=kind + cfg, **kw)
    d, batch, extra = p.make(cfg=cfg)
    c8.launch(d, batch[0], cfg)
    p.check(batch, extra)
    for b in range(B):
        db, one, _ = p.make(b, cfg=cfg)
        c8.launch(db, one[0], cfg)
        for i, (x, y) in enumerate(zip(one, batch)):
            assert torch.equal(x[0], y[b]), "batch item %d, output %d" % (b, i)
