"""RAFT update operator: motion encoder + (separable) convolutional GRU + flow and up-sampling-mask heads.

Module names follow alonet/raft/update.py (``encoder.{convc1,convc2,convf1,convf2,conv}``, ``gru.conv{z,r,q}{1,2}``,
``flow_head.{conv1,conv2}``, ``mask.{0,2}``).  ``convc1`` consumes the (B, 324, H/8, W/8) output of the correlation
lookup kernel.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

import alo_hip


def _fusable(*operands):
    """Inference on the GPU in fp32 with H*W a multiple of 4: the elementwise glue between MIOpen's convolutions (bias,
    ReLU, the GRU gates) runs as one HIP pass per stage instead of one PyTorch kernel per operation.  ``operands``: the
    activation, then every other tensor and every module the fused stage reads (alo_hip.fusable) — the passes work in place
    and have no backward, in ``train()`` mode as in ``eval()``."""
    t = operands[0]
    return alo_hip.fusable(*operands) and t.dtype == torch.float32 and (t.shape[-1] * t.shape[-2]) % 4 == 0


def _conv_act(conv, x, relu=True):
    """``act(conv(x))``: the convolution runs without bias, bias + ReLU are one in-place pass."""
    out = F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)
    if not out.is_contiguous():
        out = out.contiguous()
    return alo_hip.bias_act_nchw_(out, conv.bias, relu)


def _split_route():
    """``ALO_RAFT_CONV3X3=split``: the update block's 3x3 convolutions that ``alo_hip.conv3x3_f32`` (fp32 on the fp16 matrix cores,
    channels-last) runs faster than MIOpen — encoder.convc2, encoder.conv, flow_head.conv1, mask.0 — take it.  Opt-in; read per
    call, so a test or a benchmark run flips it in-process."""
    return os.environ.get("ALO_RAFT_CONV3X3") == "split"


_CL = torch.channels_last


def _gru_split_route():
    """``ALO_RAFT_GRU=split``: SepConvGRU runs channels-last, its 1x5 / 5x1 convolutions on ``alo_hip.conv_taps_f32`` (fp32 on the fp16
    matrix cores) and its gate passes on the channels-last flavour of alo_gru_gate / alo_gru_update.  Opt-in; read per call."""
    return os.environ.get("ALO_RAFT_GRU") == "split"


def _conv3x3_split(conv, x, relu, pad_to=None):
    """``act(conv(x))`` of a 3x3 / padding-1 ``conv`` on a channels-last fp32 ``x`` -> channels-last, bias and ReLU in the kernel's
    epilogue.  ``pad_to``: the output channels are zero-padded to that many (a multiple of 64; the padded weight and bias are
    derived once per weight version); the caller slices."""
    w, b = conv.weight, conv.bias
    if pad_to is not None and pad_to != w.shape[0]:
        w, b = alo_hip.derived(conv, f"pad{pad_to}", (conv.weight, conv.bias),
                               lambda: (F.pad(conv.weight, (0, 0, 0, 0, 0, 0, 0, pad_to - conv.weight.shape[0])).contiguous(),
                                        F.pad(conv.bias, (0, pad_to - conv.bias.shape[0])).contiguous()))
    return alo_hip.conv3x3_f32(x, w, b, relu=relu, stride=1)


def _conv1x1_to_nhwc(conv, x):
    """``relu(conv(x))`` of a 1x1 ``conv`` on an NCHW ``x`` -> channels-last: the GEMM reads x transposed instead of a copy."""
    B, C, H, W = x.shape
    w2 = conv.weight.view(conv.weight.shape[0], C)
    rows = torch.matmul(x.view(B, C, H * W).transpose(1, 2), w2.t())                     # (B, HW, Cout) = NHWC
    alo_hip.bias_act_(rows.view(B * H * W, -1), conv.bias, relu=True)
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


class FlowHead(nn.Module):
    def __init__(self, input_dim=128, hidden_dim=256, out_planes=2):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, out_planes, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x)))


def _gru_step(h, x, convz, convr, convq):
    hx = torch.cat([h, x], dim=1)
    z = torch.sigmoid(convz(hx))
    r = torch.sigmoid(convr(hx))
    q = torch.tanh(convq(torch.cat([r * h, x], dim=1)))
    return (1 - z) * h + z * q


class ConvGRU(nn.Module):
    def __init__(self, hidden_dim=128, input_dim=192 + 128):
        super().__init__()
        self.convz = nn.Conv2d(hidden_dim + input_dim, hidden_dim, 3, padding=1)
        self.convr = nn.Conv2d(hidden_dim + input_dim, hidden_dim, 3, padding=1)
        self.convq = nn.Conv2d(hidden_dim + input_dim, hidden_dim, 3, padding=1)

    def forward(self, h, x):
        return _gru_step(h, x, self.convz, self.convr, self.convq)


class SepConvGRU(nn.Module):
    """GRU with a 1x5 (horizontal) pass followed by a 5x1 (vertical) pass."""

    def __init__(self, hidden_dim=128, input_dim=192 + 128):
        super().__init__()
        c = hidden_dim + input_dim
        self.convz1 = nn.Conv2d(c, hidden_dim, (1, 5), padding=(0, 2))
        self.convr1 = nn.Conv2d(c, hidden_dim, (1, 5), padding=(0, 2))
        self.convq1 = nn.Conv2d(c, hidden_dim, (1, 5), padding=(0, 2))
        self.convz2 = nn.Conv2d(c, hidden_dim, (5, 1), padding=(2, 0))
        self.convr2 = nn.Conv2d(c, hidden_dim, (5, 1), padding=(2, 0))
        self.convq2 = nn.Conv2d(c, hidden_dim, (5, 1), padding=(2, 0))

    def forward(self, h, x):
        if _fusable(h, x, self):
            if _gru_split_route() and self.split_serves(h.shape[1], x.shape[1]):
                hx, rhx = self.split_buffers(h, x.shape[1])
                hx[:, h.shape[1]:].copy_(x)
                return self.forward_split(hx, rhx, h.shape[1]).contiguous()   # callers of this module get NCHW, as on every route
            return self._forward_fused(h, x)
        h = _gru_step(h, x, self.convz1, self.convr1, self.convq1)
        return _gru_step(h, x, self.convz2, self.convr2, self.convq2)

    def split_serves(self, C, Cx):
        """The shapes ``alo_hip.conv_taps_f32`` takes: [h | x] a multiple of 64 channels, as are C and 2C."""
        return C % 64 == 0 and (C + Cx) % 64 == 0 and self.convz1.weight.shape[:2] == (C, C + Cx)

    @staticmethod
    def split_buffers(h, Cx):
        """The channels-last [h | x] and [r*h | x] buffers of :meth:`forward_split` with ``h`` in place; the caller fills
        ``hx[:, C:]`` with x (``forward_split`` copies it to ``rhx``)."""
        B, C, H, W = h.shape
        hx = torch.empty((B, C + Cx, H, W), dtype=h.dtype, device=h.device, memory_format=_CL)
        hx[:, :C].copy_(h)
        return hx, torch.empty_like(hx)

    def forward_split(self, hx, rhx, C):
        """``_forward_fused`` channels-last (``ALO_RAFT_GRU=split``): a buffer is a (rows, C + Cx) matrix, a row per pixel; the four
        convolutions run on ``alo_hip.conv_taps_f32`` without bias and the gate passes add it.  All four launches beat what
        ``_forward_fused`` launches in their place (docs/experiments.md, "SepConvGRU on the split family").  -> net, channels-last."""
        B, Ct, H, W = hx.shape
        rows = lambda t: t.permute(0, 2, 3, 1).view(B * H * W, t.shape[1])   # noqa: E731  (a channels-last map as a matrix)
        rhx[:, C:].copy_(hx[:, C:])
        net = torch.empty((B, C, H, W), dtype=hx.dtype, device=hx.device, memory_format=_CL)
        halves = ((self.convz1, self.convr1, self.convq1), (self.convz2, self.convr2, self.convq2))
        for i, (cz, cr, cq) in enumerate(halves):
            wzr, bzr = alo_hip.derived(self, f"zr{i}", (cz.weight, cr.weight, cz.bias, cr.bias),
                                       lambda: (torch.cat([cz.weight, cr.weight], 0).contiguous(),
                                                torch.cat([cz.bias, cr.bias], 0).contiguous()))
            zr = rows(alo_hip.conv_taps_f32(hx, wzr))
            alo_hip.gru_gate_rows_(zr, bzr, rows(hx), rows(rhx), C)
            q = rows(alo_hip.conv_taps_f32(rhx, cq.weight))
            alo_hip.gru_update_rows_(q, cq.bias, zr, rows(hx), C, rows(net) if i == 1 else None)
        return net

    def _forward_fused(self, h, x):
        """Same arithmetic, different plumbing: the z and r convolutions of a pass are ONE convolution with 2C outputs,
        [h | x] and [r*h | x] live in two persistent buffers (no torch.cat), and sigmoid / tanh / gating / biases are two
        HIP passes per half (alo_gru_gate, alo_gru_update) instead of ~13 elementwise kernels."""
        B, C, H, W = h.shape
        hx = torch.empty((B, C + x.shape[1], H, W), dtype=h.dtype, device=h.device)
        rhx = torch.empty_like(hx)
        hx[:, :C].copy_(h)
        hx[:, C:].copy_(x)
        rhx[:, C:].copy_(x)
        net = torch.empty_like(h)
        halves = ((self.convz1, self.convr1, self.convq1), (self.convz2, self.convr2, self.convq2))
        for i, (cz, cr, cq) in enumerate(halves):
            wzr, bzr = alo_hip.derived(self, f"zr{i}", (cz.weight, cr.weight, cz.bias, cr.bias),
                                       lambda: (torch.cat([cz.weight, cr.weight], 0).contiguous(),
                                                torch.cat([cz.bias, cr.bias], 0).contiguous()))
            zr = F.conv2d(hx, wzr, None, cz.stride, cz.padding)
            alo_hip.gru_gate_(zr, bzr, hx, rhx, C)
            q = F.conv2d(rhx, cq.weight, None, cq.stride, cq.padding)
            alo_hip.gru_update_(q, cq.bias, zr, hx, C, net if i == 1 else None)
        return net


class SmallMotionEncoder(nn.Module):
    def __init__(self, corr_levels, corr_radius, out_planes=2):
        super().__init__()
        cor_planes = corr_levels * (2 * corr_radius + 1) ** out_planes
        self.convc1 = nn.Conv2d(cor_planes, 96, 1)
        self.convf1 = nn.Conv2d(out_planes, 64, 7, padding=3)
        self.convf2 = nn.Conv2d(64, 32, 3, padding=1)
        self.conv = nn.Conv2d(128, 80, 3, padding=1)

    def forward(self, flow, corr):
        cor = F.relu(self.convc1(corr))
        flo = F.relu(self.convf2(F.relu(self.convf1(flow))))
        out = F.relu(self.conv(torch.cat([cor, flo], dim=1)))
        return torch.cat([out, flow], dim=1)


class BasicMotionEncoder(nn.Module):
    def __init__(self, corr_levels, corr_radius, out_planes=2):
        super().__init__()
        cor_planes = corr_levels * (2 * corr_radius + 1) ** out_planes
        self.convc1 = nn.Conv2d(cor_planes, 256, 1)
        self.convc2 = nn.Conv2d(256, 192, 3, padding=1)
        self.convf1 = nn.Conv2d(out_planes, 128, 7, padding=3)
        self.convf2 = nn.Conv2d(128, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 192, 128 - out_planes, 3, padding=1)

    def _forward_split(self, flow, corr, into=None):
        """The fused route with convc2 and conv on conv3x3_f32: channels-last from convc1's GEMM (which reads the NCHW lookup
        transposed) to conv's output.  convf2 stays on MIOpen (a tie at this shape, docs/experiments.md, and its input is NCHW):
        its output turns channels-last inside the concatenation, and conv's turns NCHW inside the one with the flow — or, with
        ``into`` (a channels-last slice of SepConvGRU's [h | x] buffer), stays channels-last there."""
        B, _, H, W = flow.shape
        cor = _conv3x3_split(self.convc2, _conv1x1_to_nhwc(self.convc1, corr), True)
        flo = _conv_act(self.convf2, _conv_act(self.convf1, flow))
        x = torch.empty((B, cor.shape[1] + flo.shape[1], H, W), dtype=flow.dtype, device=flow.device, memory_format=_CL)
        x[:, :cor.shape[1]].copy_(cor)
        x[:, cor.shape[1]:].copy_(flo)
        out = _conv3x3_split(self.conv, x, True, pad_to=128)  # 126 -> 128 output channels
        k = self.conv.weight.shape[0]
        enc = torch.empty((B, k + flow.shape[1], H, W), dtype=flow.dtype, device=flow.device) if into is None else into
        enc[:, :k].copy_(out[:, :k])
        enc[:, k:].copy_(flow)
        return enc

    def forward(self, flow, corr):
        if _fusable(flow, corr, self):
            if _split_route() and corr.is_contiguous() and flow.is_contiguous():
                return self._forward_split(flow, corr)
            cor = _conv_act(self.convc2, _conv_act(self.convc1, corr))
            flo = _conv_act(self.convf2, _conv_act(self.convf1, flow))
            out = _conv_act(self.conv, torch.cat([cor, flo], dim=1))
            return torch.cat([out, flow], dim=1)
        cor = F.relu(self.convc2(F.relu(self.convc1(corr))))
        flo = F.relu(self.convf2(F.relu(self.convf1(flow))))
        out = F.relu(self.conv(torch.cat([cor, flo], dim=1)))
        return torch.cat([out, flow], dim=1)


class SmallUpdateBlock(nn.Module):
    def __init__(self, corr_levels, corr_radius, hidden_dim=96, out_planes=2):
        super().__init__()
        self.encoder = SmallMotionEncoder(corr_levels, corr_radius, out_planes=out_planes)
        self.gru = ConvGRU(hidden_dim=hidden_dim, input_dim=hidden_dim + 49)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=128, out_planes=out_planes)

    def forward(self, net, inp, corr, flow):
        inp = torch.cat([inp, self.encoder(flow, corr)], dim=1)
        net = self.gru(net, inp)
        return net, None, self.flow_head(net)


class BasicUpdateBlock(nn.Module):
    def __init__(self, corr_levels, corr_radius, hidden_dim=128, input_dim=128, out_planes=2):
        super().__init__()
        self.encoder = BasicMotionEncoder(corr_levels, corr_radius, out_planes=out_planes)
        self.gru = SepConvGRU(hidden_dim=hidden_dim, input_dim=128 + hidden_dim)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=256, out_planes=out_planes)
        self.mask = nn.Sequential(nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(256, 64 * 9, 1))

    def _gru_channels_last(self, net, inp, corr, flow):
        """Both knobs (``ALO_RAFT_CONV3X3=split`` and ``ALO_RAFT_GRU=split``): the encoder writes its channels-last output straight
        into the GRU's [h | x] buffer, and ``net`` stays channels-last from one iteration to the next and into the heads.  -> net
        (channels-last), or None when a shape or a layout is not the route's."""
        enc, C, Ci = self.encoder, net.shape[1], inp.shape[1]
        Cx = Ci + enc.conv.weight.shape[0] + flow.shape[1]
        if not (_split_route() and _gru_split_route() and _fusable(net, inp, corr, flow, self) and self.gru.split_serves(C, Cx)
                and corr.is_contiguous() and flow.is_contiguous()):
            return None
        hx, rhx = self.gru.split_buffers(net, Cx)
        hx[:, C:C + Ci].copy_(inp)
        enc._forward_split(flow, corr, into=hx[:, C + Ci:])
        return self.gru.forward_split(hx, rhx, C)

    def forward(self, net, inp, corr, flow, upsample=True):
        net_cl = self._gru_channels_last(net, inp, corr, flow)
        if net_cl is None:
            inp = torch.cat([inp, self.encoder(flow, corr)], dim=1)
            net = self.gru(net, inp)
        else:
            net = net_cl
        if _fusable(net, self.flow_head, self.mask):
            fh, m0, m2 = self.flow_head, self.mask[0], self.mask[2]
            # the 0.25 of the original RAFT (gradient balancing) is folded into the last convolution's weight and bias
            quarter = lambda: alo_hip.derived(self, "mask_quarter", (m2.weight, m2.bias), lambda: (0.25 * m2.weight, 0.25 * m2.bias))  # noqa: E731
            if _split_route() and (net.is_contiguous() or net_cl is not None):
                # net goes channels-last once for both heads (with ALO_RAFT_GRU=split it already is); flow_head.conv2 (256 -> 2: the kernel would run 64 output channels for
                # 2 and is slower than MIOpen there, docs/experiments.md) stays on F.conv2d behind one copy back to NCHW; mask.2 (1x1)
                # reads the channels-last map as the GEMM's transposed operand and writes NCHW
                B, _, H, W = net.shape
                net_cl = net.contiguous(memory_format=_CL)
                delta_flow = fh.conv2(_conv3x3_split(fh.conv1, net_cl, True).contiguous())
                m = _conv3x3_split(m0, net_cl, True).permute(0, 2, 3, 1).reshape(B, H * W, -1)          # (B, HW, 256): a view
                w2, b2 = quarter()
                up_mask = torch.baddbmm(b2.view(1, -1, 1), w2.view(1, w2.shape[0], -1).expand(B, -1, -1), m.transpose(1, 2))
                return net, up_mask.view(B, -1, H, W), delta_flow
            delta_flow = fh.conv2(_conv_act(fh.conv1, net))
            w2, b2 = quarter()
            up_mask = F.conv2d(_conv_act(m0, net), w2, b2, m2.stride, m2.padding)
            return net, up_mask, delta_flow
        delta_flow = self.flow_head(net)
        return net, 0.25 * self.mask(net), delta_flow  # 0.25: gradient balancing of the original RAFT
