"""RAFT feature / context encoders.

``BasicEncoder``: 7x7 stride-2 stem, three residual stages (64, 96, 128 channels; strides 1, 2, 2) and a 1x1 output
convolution -> features at 1/8 resolution.  Module names match alonet/raft/extractor.py:113-187 (``conv1, norm1,
layer{1,2,3}.{0,1}.{conv1,conv2,norm1,norm2,downsample.{0,1}}, conv2``) so RAFT checkpoints load unchanged.
``SmallEncoder`` is the bottleneck variant used by RAFT-small.

By default every layer is a stock PyTorch-ROCm op.  ``ALO_RAFT_ENCODER=split`` (opt-in, read per call, independent of
``ALO_RAFT_CONV3X3`` / ``ALO_RAFT_GRU``) sends a ``BasicEncoder`` at inference in fp32 on the GPU through the library instead
(:meth:`BasicEncoder._forward_split`): the map is channels-last from the stem's output to ``conv2``'s, the 3x3 convolutions run on
``alo_hip.conv3x3_f32`` and the 1x1 ones on ``alo_hip.conv1x1_strided_f32`` (fp32 on the fp16 matrix cores) wherever they were
measured faster than MIOpen, ``InstanceNorm2d`` (+ ReLU) is ``alo_hip.instancenorm_nhwc_f32`` in place, an eval-mode
``BatchNorm2d`` is folded into its convolution, and the 96-channel stage runs zero-padded to 128 channels.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

import alo_hip

_CL = torch.channels_last


def _encoder_split_route():
    """``ALO_RAFT_ENCODER=split``: a BasicEncoder at inference takes :meth:`BasicEncoder._forward_split`.  Opt-in; read per call, so a
    test or a benchmark run flips it in-process."""
    return os.environ.get("ALO_RAFT_ENCODER") == "split"


def _pad64(channels):
    return (channels + 63) // 64 * 64


# (Cin, Cout, stride), padded, of the 3x3 convolutions that conv3x3_f32 does NOT run faster than MIOpen on a channels-last map at the
# RAFT leg's shapes (8 and 4 frames of 1280x720; docs/experiments.md, "RAFT encoders on the split family"): they stay on F.conv2d
# inside the route.  layer3.0.conv1 (96 -> 128 at 180x320, stride 2): 0.378 against 0.346 ms at 8 frames, 0.193 against 0.189 at 4.
_CONV3X3_ON_MIOPEN = {(128, 128, 2)}


def _route_weights(conv, bn=None):
    """``(w, b)`` of ``conv`` as the route runs it, derived once per version of its sources (``alo_hip.derived``): an eval-mode
    ``bn`` behind it folded in (fp32: ``w * scale``, ``(b - running_mean) * scale + beta`` with ``scale = gamma / sqrt(var + eps)``,
    the fold of alonet/detr/backbone.py), then input and output channels zero-padded to multiples of 64 — a padding channel is
    exactly 0 through convolution, norm, ReLU and add — and a 1x1 weight as a (Cout, Cin) matrix."""
    sources = (conv.weight, conv.bias) if bn is None else (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)

    def build():
        w, b = conv.weight.float(), conv.bias.float()
        if bn is not None:
            scale = bn.weight.float() * (bn.running_var.float() + bn.eps).rsqrt()
            w, b = w * scale.view(-1, 1, 1, 1), (b - bn.running_mean.float()) * scale + bn.bias.float()
        cout, cin = w.shape[:2]
        if cin >= 64:     # (the stem's 3 input channels stay 3)
            w = F.pad(w, (0, 0, 0, 0, 0, _pad64(cin) - cin))
        w, b = F.pad(w, (0, 0, 0, 0, 0, 0, 0, _pad64(cout) - cout)), F.pad(b, (0, _pad64(cout) - cout))
        w = w.reshape(w.shape[0], w.shape[1]) if w.shape[2:] == (1, 1) else w.contiguous(memory_format=_CL)
        return w.contiguous() if w.dim() == 2 else w, b.contiguous()

    return alo_hip.derived(conv, "raft_encoder_route" if bn is None else "raft_encoder_route_bn", sources, build)


def _norm(kind, channels, groups=None):
    if kind == "group":
        return nn.GroupNorm(num_groups=groups or channels // 8, num_channels=channels)
    if kind == "batch":
        return nn.BatchNorm2d(channels)
    if kind == "instance":
        return nn.InstanceNorm2d(channels)
    if kind == "none":
        return nn.Sequential()
    raise ValueError(f"unknown norm_fn {kind!r}")


class ResidualBlock(nn.Module):
    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = _norm(norm_fn, planes, planes // 8)
        self.norm2 = _norm(norm_fn, planes, planes // 8)
        self.downsample = None
        if stride != 1:
            self.norm3 = _norm(norm_fn, planes, planes // 8)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class BottleneckBlock(nn.Module):
    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__()
        mid = planes // 4
        self.conv1 = nn.Conv2d(in_planes, mid, 1)
        self.conv2 = nn.Conv2d(mid, mid, 3, padding=1, stride=stride)
        self.conv3 = nn.Conv2d(mid, planes, 1)
        self.relu = nn.ReLU(inplace=True)
        groups = planes // 8
        self.norm1 = _norm(norm_fn, mid, groups)
        self.norm2 = _norm(norm_fn, mid, groups)
        self.norm3 = _norm(norm_fn, planes, groups)
        self.downsample = None
        if stride != 1:
            self.norm4 = _norm(norm_fn, planes, groups)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride), self.norm4)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        y = self.relu(self.norm3(self.conv3(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class _Encoder(nn.Module):
    block = None
    widths = None

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0):
        super().__init__()
        self.norm_fn = norm_fn
        w0, w1, w2 = self.widths
        self.norm1 = _norm(norm_fn, w0, 8)
        self.conv1 = nn.Conv2d(3, w0, 7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = w0
        self.layer1 = self._make_layer(w0, stride=1)
        self.layer2 = self._make_layer(w1, stride=2)
        self.layer3 = self._make_layer(w2, stride=2)
        self.conv2 = nn.Conv2d(w2, output_dim, 1)
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _make_layer(self, dim, stride=1):
        layers = (self.block(self.in_planes, dim, self.norm_fn, stride=stride), self.block(dim, dim, self.norm_fn, 1))
        self.in_planes = dim
        return nn.Sequential(*layers)

    def forward(self, x):
        pair = isinstance(x, (tuple, list))  # two frames share one pass: stacked on the batch axis
        if pair:
            n = x[0].shape[0]
            x = torch.cat(x, dim=0)
        if _encoder_split_route() and self._split_serves(x):
            x = self._forward_split(x)
        else:
            x = self.relu1(self.norm1(self.conv1(x)))
            x = self.conv2(self.layer3(self.layer2(self.layer1(x))))
        if self.training and self.dropout is not None:
            x = self.dropout(x)
        return torch.split(x, [n, n], dim=0) if pair else x

    def _split_serves(self, x):
        return False


class BasicEncoder(_Encoder):
    block = ResidualBlock
    widths = (64, 96, 128)

    def _split_serves(self, x):
        """The gate of ``ALO_RAFT_ENCODER=split``: inference (grad mode off, no dropout to apply) on a 4-D fp32 CUDA batch; every
        norm an ``InstanceNorm2d`` as ``nn.InstanceNorm2d(c)`` makes it (no affine, no running statistics), or every norm a
        ``BatchNorm2d`` in eval mode; widths the kernels take once padded to multiples of 64."""
        norms = [m for m in self.modules() if isinstance(m, (nn.InstanceNorm2d, nn.BatchNorm2d, nn.GroupNorm))]
        if self.norm_fn == "instance":
            ok = all(isinstance(m, nn.InstanceNorm2d) and not m.affine and not m.track_running_stats for m in norms)
        elif self.norm_fn == "batch":
            ok = all(isinstance(m, nn.BatchNorm2d) and not m.training and m.affine and m.track_running_stats for m in norms)
        else:
            ok = False
        return (ok and x.dim() == 4 and x.dtype == torch.float32 and alo_hip.fusable(x, self) and not torch.is_grad_enabled()
                and not (self.training and self.dropout is not None) and max(self.widths) <= 256
                and self.conv2.weight.shape[0] % 64 == 0 and self.conv1.weight.dtype == torch.float32)

    def _conv3x3(self, conv, bn, x, relu):
        """``act(bn?(conv(x)))`` of a 3x3 ``conv`` on the route's channels-last map: bias (and the folded ``bn``) and ReLU in the
        epilogue of ``alo_hip.conv3x3_f32`` — or, for the shapes of ``_CONV3X3_ON_MIOPEN``, MIOpen on the same padded tensors."""
        w, b = _route_weights(conv, bn)
        stride = conv.stride[0]
        if (w.shape[1], w.shape[0], stride) in _CONV3X3_ON_MIOPEN:
            y = F.conv2d(x, w, b, stride, 1).contiguous(memory_format=_CL)
            return torch.relu_(y) if relu else y
        return alo_hip.conv3x3_f32(x, w, b, relu=relu, stride=stride)

    def _block_split(self, blk, x):
        """A ResidualBlock on the route.  instance: convolution, then norm + ReLU in place; batch (eval): the norm is in the
        convolution's weights, bias and ReLU in its epilogue.  ``relu(x + y)`` is two in-place torch passes."""
        instance = self.norm_fn == "instance"
        bn = (lambda m: None) if instance else (lambda m: m)
        y = self._conv3x3(blk.conv1, bn(blk.norm1), x, relu=not instance)
        if instance:
            alo_hip.instancenorm_nhwc_f32(y, blk.norm1.eps, relu=True, out=y)
        y = self._conv3x3(blk.conv2, bn(blk.norm2), y, relu=not instance)
        if instance:
            alo_hip.instancenorm_nhwc_f32(y, blk.norm2.eps, relu=True, out=y)
        if blk.downsample is not None:
            down = blk.downsample[0]
            w, b = _route_weights(down, bn(blk.downsample[1]))
            x = alo_hip.conv1x1_strided_f32(x, w, b, down.stride[0])
            if instance:
                alo_hip.instancenorm_nhwc_f32(x, blk.downsample[1].eps, out=x)
        return torch.relu_(y.add_(x))

    def _forward_split(self, x):
        """``ALO_RAFT_ENCODER=split``: the stem on MIOpen with a channels-last image (its output is then channels-last), the blocks
        as :meth:`_block_split` runs them, ``conv2`` on the 1x1 kernel.  Which convolutions run where was decided per layer at the
        RAFT leg's shapes (docs/experiments.md, "RAFT encoders on the split family").  -> NCHW-contiguous, as on the stock ops."""
        instance = self.norm_fn == "instance"
        w, b = _route_weights(self.conv1, None if instance else self.norm1)
        x = F.conv2d(x.contiguous(memory_format=_CL), w, b, self.conv1.stride, self.conv1.padding).contiguous(memory_format=_CL)
        if instance:
            alo_hip.instancenorm_nhwc_f32(x, self.norm1.eps, relu=True, out=x)
        else:
            torch.relu_(x)
        for layer in (self.layer1, self.layer2, self.layer3):
            for blk in layer:
                x = self._block_split(blk, x)
        w, b = _route_weights(self.conv2)
        return alo_hip.conv1x1_strided_f32(x, w, b, 1).contiguous()


class SmallEncoder(_Encoder):
    block = BottleneckBlock
    widths = (32, 64, 96)
