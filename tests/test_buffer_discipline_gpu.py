"""Every launch stays in its buffers and ignores stale bytes: the entry points of ``libalo_hotpath.so`` under tests/guarded.py.

Per-kernel sweep: each case calls a public wrapper under ``GuardedLaunches`` (every launch then runs twice between guard zones, its
outputs and workspaces pre-filled with 0xFF and with 0x3C bytes; see guarded.py for what is checked), asserts that the entry points it
is there for were launched, and then applies the reference check the suite already has for that op — the helpers of the other test
modules, at their bounds; where no fp64 helper exists the guarded result equals the un-guarded call bit for bit.  Shapes are the
smallest with a partial last tile in every tiled dimension and, where there is a batch, an item boundary inside a tile; the tile
constant is named on each row.  Whole models then run one small forward each under the same guard.

Where a starting shape cannot reach its kernel through the wrapper the row says what was taken instead:
  * linear_packed: the wrapper takes K >= 512 (K = 256 belongs to linear_shortk), so K = 512.
"""
import numpy as np
import pytest
import torch

import alo_hip
import kernel_bounds as kb
import oracle as O
from guarded import ROLES, GuardedLaunches
from helpers import level_start, msda_case
from kernel_bounds import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
NAMES = {F32: "fp32", F64: "fp64", BF16: "bf16", F16: "fp16"}
CASES = []


def case(name, *expects):
    def add(thunk):
        CASES.append(pytest.param(thunk, frozenset(expects), id=name))
        return thunk
    return add


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand16(g, dtype, *shape, scale=1.0):
    """Random 16-bit operands; fp16 ones without subnormals (what test_layers_f16_gpu.py's bounds assume)."""
    t = torch.randn(*shape, device=DEV, generator=g) * scale
    if dtype == F16:
        from test_layers_f16_gpu import h16
        return h16(t)
    return t.to(dtype)


def to16(t, dtype):
    if dtype == F16:
        from test_layers_f16_gpu import h16
        return h16(t)
    return t.to(dtype)


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert torch.equal(bits(got), bits(want)), f"{what}: the guarded result differs from the un-guarded call"


# ---- linears and FFN ---------------------------------------------------------------------------------------------------------------
def check_linear_any(dtype, x2, w, b, relu, res, got, what):
    if dtype == BF16:
        from test_backbone_kernels_gpu import check_linear
        check_linear(x2, w, b, relu, res, got, what)
    else:
        from test_layers_f16_gpu import linear_ref_and_bound
        ref, bound = linear_ref_and_bound(x2, w, b, relu, res)
        compare(got, ref, bound, what)


def _linear_case(kind, dtype, m, n, k):
    # gemm.hip: kRows = 64 rows per tile, 256 output columns per pass; M = 65: one full tile and a tile of one row
    def thunk(guard):
        g = gen(m * 1000 + n + k)
        x, w, b, res = rand16(g, dtype, m, k), rand16(g, dtype, n, k, scale=k ** -0.5), rand16(g, dtype, n, scale=0.5), rand16(g, dtype, m, n)
        fn = alo_hip.linear_shortk if kind == "shortk" else alo_hip.linear_packed
        got = guard(lambda: fn(x, w, b, True, residual=res))
        return lambda: check_linear_any(dtype, x, w, b, True, res, got, f"linear_{kind} {NAMES[dtype]} {m, n, k}")
    expects = ("alo_linear_shortk",) if kind == "shortk" else ("alo_linear_packed", "alo_pack_mfma_b")
    case(f"linear_{kind}-{NAMES[dtype]}-M{m}-N{n}-K{k}", *expects)(thunk)


for _dt in (BF16, F16):
    for _m in (1, 65):
        for _n, _k in ((64, 64), (320, 128), (64, 256)):
            _linear_case("shortk", _dt, _m, _n, _k)
        _linear_case("packed", _dt, _m, 128, 512)   # gemm_packed.hip: 64-row tiles, 128-column blocks; K = 512: the wrapper's smallest


def _conv1x1_case(cin, cout, h, w, packed):
    # the tile loader of linear_shortk / linear_packed (64 pixel rows) addressing pixel (n, 2 yo, 2 xo): 2 x 4 x 3 = 24 kept pixels of a
    # 5 x 7 map, 2 of a 1 x 1 map; two images, so the item boundary falls inside the one tile
    def thunk(guard):
        from test_backbone_kernels_gpu import check_linear
        g = gen(cin + cout + h)
        x = torch.randn(2, cin, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
        wt, b = rand16(g, BF16, cout, cin, scale=cin ** -0.5), rand16(g, BF16, cout, scale=0.5)
        assert alo_hip.linear_shortk_supported(x.permute(0, 2, 3, 1), wt) == (not packed)
        got = guard(lambda: alo_hip.conv1x1_strided(x, wt, b, 2, relu=True))   # raises unless conv1x1_strided_supported (under no_grad)
        rows = x[:, :, ::2, ::2].permute(0, 2, 3, 1).reshape(-1, cin)
        return lambda: check_linear(rows, wt, b, True, None, got.permute(0, 2, 3, 1).reshape(-1, cout), "conv1x1_strided")
    case(f"conv1x1_strided-{'packed' if packed else 'unpacked'}-{cin}to{cout}-{h}x{w}", "alo_conv1x1_nhwc",
         *(("alo_pack_mfma_b",) if packed else ()))(thunk)


for _h, _w in ((5, 7), (1, 1)):
    _conv1x1_case(64, 64, _h, _w, False)
    _conv1x1_case(512, 128, _h, _w, True)


def _ffn_case(dtype, m, fh):
    # gemm.hip ffn256: 64 rows at a time in LDS, the hidden width in 256-column passes
    def thunk(guard):
        g = gen(m + fh)
        x = rand16(g, dtype, m, 256)
        w1, w2 = rand16(g, dtype, fh, 256, scale=0.06), rand16(g, dtype, 256, fh, scale=0.03)
        b1, b2 = rand16(g, dtype, fh), rand16(g, dtype, 256)
        got = guard(lambda: alo_hip.ffn256(x, w1, b1, w2, b2))

        def check():
            if dtype == F16:
                from test_layers_f16_gpu import ffn_ref_and_bound
                ref, bound = ffn_ref_and_bound(x, w1, b1, w2, b2)
                compare(got, ref, bound, f"ffn256 fp16 M={m} F={fh}")
            else:   # no fp64 helper for bf16
                same_bits(got, alo_hip.ffn256(x, w1, b1, w2, b2), f"ffn256 bf16 M={m} F={fh}")
        return check
    case(f"ffn256-{NAMES[dtype]}-M{m}-F{fh}", "alo_ffn256", "alo_pack_mfma_b")(thunk)


for _dt in (BF16, F16):
    for _m in (1, 65):
        for _fh in (256, 512):
            _ffn_case(_dt, _m, _fh)


# ---- attention-side layers ---------------------------------------------------------------------------------------------------------
def _mask(g, n, s):
    mask = torch.rand(n, s, device=DEV, generator=g) < 0.3
    mask[0, 0], mask[-1, -1] = True, False
    return mask


def _value_proj_case(dtype):
    # gemm.hip: 64-row tiles over N * S = 130 rows: the image boundary (row 65) falls inside the second tile
    def thunk(guard):
        g = gen(65)
        x, w, b = rand16(g, dtype, 2, 65, 64), rand16(g, dtype, 64, 64, scale=0.1), rand16(g, dtype, 64)
        mask = _mask(g, 2, 65)
        got = guard(lambda: alo_hip.value_proj_head_major(x, w, b, mask, 2))

        def check():   # as test_layers_f16_gpu / test_fused_gpu: the two-step chain, bit for bit
            two_step = alo_hip.value_head_major(alo_hip.linear_shortk(x, w, b).view(2, 65, 2, 32), mask)
            assert got.shape == (2, 2, 65, 32) and torch.equal(got, two_step)
        return check
    case(f"value_proj_head_major-{NAMES[dtype]}", "alo_value_proj_head_major")(thunk)


def _value_hm_case(dtype):
    # fused.hip value_head_major_kernel: 64 pixels per block; S = 65
    def thunk(guard):
        g = gen(8)
        value, mask = rand16(g, dtype, 2, 65, 2, 8), _mask(g, 2, 65)
        got = guard(lambda: alo_hip.value_head_major(value, mask))
        return lambda: same_bits(got, value.masked_fill(mask[..., None, None], 0).permute(0, 2, 1, 3).contiguous(), "value_head_major")
    case(f"value_head_major-{NAMES[dtype]}", "alo_value_head_major")(thunk)


for _dt in (BF16, F16):
    _value_proj_case(_dt)
    _value_hm_case(_dt)


def _encoder_block_case(form):
    # encoder_block.hip: 64-row tiles over 2 x 65 rows, F = 256: one pass of the hidden width
    def thunk(guard):
        from test_encoder_block_gpu import _assert_same, _block, _chain, _inputs
        cpu = torch.Generator().manual_seed(11)
        r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=cpu) * scale).to(DEV, BF16)   # noqa: E731
        w = dict(wo=r(256, 256, scale=1 / 16), bo=r(256, scale=0.5), g1=1 + r(256, scale=0.3), e1=r(256, scale=0.3),
                 w1=r(256, 256, scale=1 / 16), b1=r(256, scale=0.5), w2=r(256, 256, scale=1 / 16), b2=r(256, scale=0.5),
                 g2=1 + r(256, scale=0.3), e2=r(256, scale=0.3),
                 wv=r(256, 256, scale=1 / 16), bv=r(256, scale=0.5), wq=r(384, 256, scale=1 / 16), bq=r(384, scale=0.5))
        args = _inputs(2, 65, seed=265, mask="proj" in form)
        got = guard(lambda: _block(form, w, *args))
        return lambda: _assert_same(got, _chain(form, w, *args), form)
    case(f"encoder_block-{form}", "alo_encoder_block", "alo_pack_mfma_b")(thunk)


for _form in ("ffn", "ffn+proj", "tail+ffn", "tail+ffn+proj"):
    _encoder_block_case(_form)


# ---- elementwise glue --------------------------------------------------------------------------------------------------------------
def _ln_check_any(dtype, out, x, res, gamma, beta, what):
    if dtype == F16:   # the bound of test_layers_f16_gpu.test_add_layernorm_fp16
        from test_layers_f16_gpu import RND, TINY
        ref, bound = kb.layernorm_ref_and_bound(x.float() + res.float(), gamma.float(), beta.float(), 1e-5, bf16=False)
        compare(out, ref, bound + RND * ref.abs() + TINY, what)
    else:
        from test_glue_kernels_gpu import _ln_check
        _ln_check(out, x, res, gamma, beta, dtype, None, what)


def _layernorm_case(dtype, rows, c):
    # fused.hip add_layernorm_kernel: one wave per row, 4 rows per block, 256 channels per chunk: C = 64 leaves lanes idle, C = 260 has
    # a second chunk of one lane; rows = 7: a block of 3 rows
    def thunk(guard):
        x, res, gamma, beta, _ = kb.layernorm_inputs(rows, c, DEV, seed=rows * 7 + c)
        x, res, gamma, beta = (to16(t, dtype) for t in (x, res, gamma, beta))
        pos = rand16(gen(rows + c), dtype, rows, c)
        out, out_pos = guard(lambda: alo_hip.add_layernorm(x, res, gamma, beta, 1e-5, pos=pos))

        def check():
            assert torch.equal(out_pos, out + pos)
            _ln_check_any(dtype, out, x, res, gamma, beta, f"add_layernorm {NAMES[dtype]} rows={rows} C={c}")
        return check
    case(f"add_layernorm-{NAMES[dtype]}-rows{rows}-C{c}", "alo_add_layernorm")(thunk)


for _dt in (F32, BF16, F16):
    for _rows in (1, 7):
        for _c in (64, 260):
            _layernorm_case(_dt, _rows, _c)


@case("add_layernorm-bf16-out-aliases-x", "alo_add_layernorm")
def _(guard):
    """"`out` may alias `x`" (include/alo_hotpath.h): the wrapper never does it, so the entry point is launched directly."""
    x, res, gamma, beta, _ = kb.layernorm_inputs(7, 260, DEV, seed=3)
    x, res, gamma, beta = x.bfloat16(), res.bfloat16(), gamma.bfloat16(), beta.bfloat16()
    x2 = x.clone()
    guard(lambda: alo_hip._launch("alo_add_layernorm", x2.device, "add_layernorm/rows=7", 0.0, 0.0, x2, res, gamma, beta, x2, None, None,
                                  7, 260, 1e-5, alo_hip.ALO_BF16))
    return lambda: same_bits(x2, alo_hip.add_layernorm(x, res, gamma, beta, 1e-5), "add_layernorm in place")


def _bias_act_case(dtype):
    # fused.hip bias_act_kernel: 4 elements per thread, 256 threads per block: 7 x 64 / 4 = 112 threads of one block
    def thunk(guard):
        g = gen(31)
        x = (torch.randn(7, 64, device=DEV, generator=g)).to(dtype)
        bias, res = torch.randn(64, device=DEV, generator=g).to(dtype), torch.randn(7, 64, device=DEV, generator=g).to(dtype)
        x0 = x.clone()
        got = guard(lambda: alo_hip.bias_act_(x, bias, res, True))

        def check():
            assert got.data_ptr() == x.data_ptr()
            same_bits(got, alo_hip.bias_act_(x0.clone(), bias, res, True), "bias_act_")
            want = torch.relu(x0.double() + bias.double() + res.double())
            assert (got.double() - want).abs().max().item() <= 2.0 ** -8 * max(1.0, want.abs().max().item())
        return check
    case(f"bias_act-{NAMES[dtype]}-rows7", "alo_bias_act")(thunk)


for _dt in (F32, BF16, F16):
    _bias_act_case(_dt)


@case("bias_act_nchw-2x3xHW4", "alo_bias_act_nchw")
def _(guard):
    # fused.hip: one float4 per thread, HW % 4 == 0: (2, 3, 2 x 2) is 6 vectors, one per (item, channel)
    g = gen(5)
    x, bias = torch.randn(2, 3, 2, 2, device=DEV, generator=g), torch.randn(3, device=DEV, generator=g)
    ref = torch.relu(x.double() + bias.double().view(1, -1, 1, 1))
    got = guard(lambda: alo_hip.bias_act_nchw_(x, bias, True))
    return lambda: compare(got, ref, 2.0 ** -24 * ref.abs(), "bias_act_nchw")   # the bound of test_bias_act_nchw_at_raft_size


@case("gru_gate+gru_update-B2-C4-HW12", "alo_gru_gate", "alo_gru_update")
def _(guard):
    # fused.hip: float4 per thread over B x C x HW / 4; h and r * h are the first C = 4 channels of (2, 4 + 3, 3, 4) buffers, so the
    # channels past C of both (and the r half of zr) are bytes the kernels must leave alone
    from test_glue_kernels_gpu import _gru_buffers, _gru_round_trip
    zr, hx, rhx, q, bzr, bq = _gru_buffers(2, 4, 3, 3, 4, seed=6)
    assert hx.stride(0) != 4 * 12
    guard(lambda: _gru_round_trip(zr, hx, rhx, q, bzr, bq, 4, "gru B=2 C=4"))   # the helper checks as it goes (and passes `net`)
    return lambda: None


def _pos_case(dtype):
    # fused.hip pos_prefix_kernel: 64 columns per item (W = 65: two items, the second of one column); pos_generate_kernel: float4s
    def thunk(guard):
        shapes, b, nf = [(5, 65), (3, 33), (2, 17), (1, 9)], 2, 128
        if dtype != F16:
            from test_glue_kernels_gpu import _check_pos
            guard(lambda: _check_pos(b, shapes, nf, dtype, True, True, ["corner", "scatter+right"], seed=14))   # the helper calls and checks
            return lambda: None
        from alonet.transformers import PositionEmbeddingSine
        from test_layers_f16_gpu import RND, TINY
        enc = PositionEmbeddingSine(nf, normalize=True, center=True)
        level_embed = rand16(gen(5), F16, len(shapes), 2 * nf)
        mask_flat = kb.pyramid_masks(b, shapes, ["corner", "scatter+right"], DEV, seed=14)
        sh = torch.tensor(shapes, dtype=torch.int32, device=DEV)
        start = torch.from_numpy(level_start(shapes)).to(DEV)
        dim_t = enc.dim_t(torch.device(DEV))
        got = guard(lambda: alo_hip.pos_sine_flat(mask_flat, sh, start, dim_t, level_embed, True, True, enc.scale, F16))

        def check():   # the bound of test_layers_f16_gpu.test_pos_sine_flat_fp16
            ref, p = kb.pos_sine_ref(mask_flat, shapes, dim_t, level_embed, True, True, enc.scale)
            compare(got, ref, kb.pos_sine_bound(ref, p) + RND * ref.abs() + TINY, "pos_sine_flat fp16")
        return check
    case(f"pos_sine_flat-{NAMES[dtype]}", "alo_pos_sine_flat")(thunk)


for _dt in (F32, BF16, F16):
    _pos_case(_dt)


# ---- convolutions and stem -----------------------------------------------------------------------------------------------------------
def _conv3x3_case(n, cin, cout, h, w, stride, note, workspace=False):
    # conv.hip: kPix = 64 output pixels per tile, 128 output columns per block (64 on the register path of the 64-channel layers)
    def thunk(guard):
        from test_backbone_kernels_gpu import _conv_operands, check_conv3x3
        assert bool(alo_hip.lib().alo_conv3x3_workspace_bytes(n, h, w, cin, cout, stride)) == workspace
        x, wt, b = _conv_operands(n, cin, cout, h, w, seed=cin + cout + h)
        got = guard(lambda: alo_hip.conv3x3(x, wt, b, relu=True, stride=stride))
        return lambda: check_conv3x3(x, wt, b, True, stride, got, f"conv3x3 {n, cin, cout, h, w} s={stride}")
    case(f"conv3x3-bf16-{note}-{n}x{cin}to{cout}x{h}x{w}-s{stride}", "alo_conv3x3_nhwc", "alo_pack_mfma_b")(thunk)


for _s in (1, 2):
    _conv3x3_case(2, 64, 64, 5, 7, _s, "c64-registers")     # 35 (12 at stride 2) pixels per image: two partial tiles
    _conv3x3_case(1, 128, 64, 1, 1, _s, "generic")          # one pixel: every tap but the centre is padding
    _conv3x3_case(2, 128, 128, 9, 9, _s, "generic")         # 81 pixels: a full tile and a partial one per image
_conv3x3_case(1, 256, 128, 9, 9, 1, "split-k", workspace=True)   # SPLITK_CONV[0]: z = 2, fp32 partial sums in the workspace


def _conv_f32_case(stride):
    # conv_f32.hip: 64-pixel tiles; MAG_SHAPE (2, 128 -> 64, 5 x 7): rows shorter than a tile, a tile crossing row ends and images
    def thunk(guard):
        from conv_f32_ref import reference_and_bound
        from test_conv3x3_f32_gpu import MAG_SHAPE, _operands, _run
        x, wt, b = _operands(MAG_SHAPE)
        got = guard(lambda: _run(x, wt, b, stride, True))

        def check():
            ref, bound = reference_and_bound(x, wt, b, stride, True)
            compare(got, ref, bound, f"conv3x3_f32 stride {stride}")
        return check
    case(f"conv3x3_f32-2x128to64x5x7-s{stride}", "alo_conv3x3_nhwc", "alo_pack_mfma_b")(thunk)


for _s in (1, 2):
    _conv_f32_case(_s)


def _small_conv_case(n, cin, cout, h, w):
    # conv_small.hip: 8 x 16 pixel tiles: 9 x 17 and 7 x 15 leave a partial tile (or a tile of one row / column) in both directions
    def thunk(guard):
        from test_glue_kernels_gpu import _small_conv, _small_conv_check
        conv, g = _small_conv(cin, cout, True, h * w + cin)
        x = torch.randn(n, cin, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
        guard(lambda: _small_conv_check(x, conv, f"conv3x3_small {cin}->{cout} {h} x {w}"))   # the helper calls and checks
        return lambda: None
    case(f"conv3x3_small-{n}x{cin}to{cout}x{h}x{w}", "alo_conv3x3_small_nhwc")(thunk)


_small_conv_case(2, 16, 1, 9, 17)
_small_conv_case(1, 64, 32, 7, 15)


def _stem_case(shape, layout):
    # stem.hip: tiles of 8 x 7 pooled pixels: (37, 53) pools to 10 x 14, i.e. 2 x 2 tiles with a partial second row; (8, 8) to 2 x 2
    def thunk(guard):
        from test_backbone_kernels_gpu import _stem_operands, check_stem
        g, wt, b = _stem_operands(sum(shape))
        x = torch.randn(shape, device=DEV, generator=g).bfloat16()
        if layout == "nhwc":
            x = x.contiguous(memory_format=torch.channels_last)
        got = guard(lambda: alo_hip.stem_conv_pool(x, wt, b))
        return lambda: check_stem(x, wt, b, got, f"stem {shape} {layout}")
    case(f"stem_conv_pool-{'x'.join(map(str, shape))}-{layout}", "alo_stem_conv_pool", "alo_pack_mfma_b")(thunk)


_stem_case((2, 3, 37, 53), "nchw")
_stem_case((2, 3, 37, 53), "nhwc")
_stem_case((1, 3, 8, 8), "nchw")


# ---- norms and geometry --------------------------------------------------------------------------------------------------------------
@case("groupnorm_rows-B2-HW257-C256-into-a-flat-buffer", "alo_groupnorm_rows")
def _(guard):
    # groupnorm.hip: kGnRows = 256 rows per chunk: HW = 257 is a chunk and a chunk of one row.  The output is a slice of a flat
    # (2, 3 + 257 + 5, 256) buffer: batch stride > HW * C, and the rows either side of the slice are gaps the kernel must not touch
    from test_glue_kernels_gpu import _gn_params, _gn_rows_check
    g = gen(2)
    gamma, beta = _gn_params(256, 1)
    x = (torch.randn(2, 257, 256, device=DEV, generator=g) * 3 + 0.7).bfloat16()
    flat = torch.full((2, 3 + 257 + 5, 256), 7.0, device=DEV, dtype=BF16)
    out = guard(lambda: alo_hip.groupnorm_rows(x, gamma, beta, 32, 1e-5, out=flat[:, 3:3 + 257]))

    def check():
        assert out.data_ptr() == flat[:, 3:].data_ptr() and out.stride(0) == 265 * 256
        _gn_rows_check(flat[:, 3:260], x, 32, gamma, beta, "groupnorm_rows HW=257")
        assert (flat[:, :3] == 7.0).all() and (flat[:, 260:] == 7.0).all()
    return check


@case("groupnorm_nhwc-2x16x5x7-8-groups-relu", "alo_groupnorm_rows_act")
def _(guard):
    # groupnorm.hip: 256-row chunks (35 rows: one partial chunk per image), 2 channels per group: a thread's 8 channels span 4 groups
    g = gen(16)
    x = (torch.randn(2, 16, 5, 7, device=DEV, generator=g) * 2 + 0.3).bfloat16().contiguous(memory_format=torch.channels_last)
    norm = torch.nn.GroupNorm(8, 16).to(DEV).to(BF16)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(16, device=DEV, generator=g))
        norm.bias.copy_(torch.randn(16, device=DEV, generator=g))
    out = guard(lambda: alo_hip.groupnorm_nhwc(x, norm, relu=True))

    def check():
        ref, bound = kb.groupnorm_ref_and_bound(x, 8, norm.weight.detach(), norm.bias.detach(), norm.eps, True)
        compare(out, ref, bound, "groupnorm_nhwc")
    return check


@case("upsample_add-B3-Q1-C8-4x4-to-9x7", "alo_upsample_add_nhwc")
def _(guard):
    # groupnorm.hip alo_upsample_add_nhwc: one 16-byte vector (8 channels) per thread: 3 x 63 threads of one block
    from test_glue_kernels_gpu import _upadd_stock
    g = gen(4)
    x = torch.randn(3, 8, 4, 4, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    fpn = torch.randn(3, 8, 9, 7, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    got = guard(lambda: alo_hip.upsample_add(x, fpn))
    return lambda: same_bits(got, torch.cat([_upadd_stock(x, fpn, 1, i) for i in range(3)]).contiguous(memory_format=torch.channels_last),
                             "upsample_add against the stock ops")


@case("mask_pyramid+encoder_reference_points-B2-33x65", "alo_mask_pyramid", "alo_encoder_reference_points")
def _(guard):
    # geometry.hip: 256-thread blocks over B x S = 2 x 68 level pixels; a 33 x 65 frame's levels at strides 8 .. 64, the last one nearest
    from alonet.deformable_detr.deformable_transformer import DeformableTransformerEncoder, _level_geometry
    from test_fused_gpu import _stock_masks
    shapes = [(5, 9), (3, 5), (2, 3), (1, 2)]
    mask = torch.zeros(2, 1, 33, 65, device=DEV)
    mask[1, :, 20:, :], mask[1, :, :, 50:] = 1, 1
    got_m, got_r = guard(lambda: alo_hip.mask_pyramid(mask, shapes, nearest_levels=[3]))
    spatial_shapes, _ = _level_geometry(tuple(shapes), torch.device(DEV))
    points = guard(lambda: alo_hip.encoder_reference_points(got_r, shapes))

    def check():
        want_m, want_r = _stock_masks(mask, shapes, 3)
        assert torch.equal(got_m, want_m) and torch.equal(got_r, want_r)
        want = DeformableTransformerEncoder.get_reference_points(spatial_shapes, got_r, device=got_r.device, is_tracing=True)
        assert torch.equal(points, want)
    return check


@case("panoptic_onehot-2x3-5x7-to-11x13", "alo_panoptic_onehot")
def _(guard):
    # geometry.hip alo_panoptic_onehot: 256-thread blocks over B x H x W = 2 x 143 output pixels: the image boundary falls inside a block
    from test_glue_kernels_gpu import _onehot_check
    logits = torch.randn(2, 3, 5, 7, device=DEV, generator=gen(203)) * 3
    logits[:, :, :2] -= 6.0
    got = guard(lambda: alo_hip.panoptic_onehot(logits, (11, 13), 0.5))
    return lambda: _onehot_check(logits, (11, 13), got, "panoptic_onehot 5 x 7 -> 11 x 13")


# ---- MSDA (16-byte aligned pointers) ---------------------------------------------------------------------------------------------------
SMALL_L2 = [(5, 7), (3, 4)]                     # P = 3: the generic kernels' runtime L * P loop
SMALL_L4 = [(5, 7), (3, 4), (2, 3), (1, 2)]     # L = P = 4: the unrolled 16-sample stage; bf16 / D = 32 takes the matrix-pipe kernel
NP = {F32: np.float32, F64: np.float64}


def dev(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x.to(dtype) if dtype is not None else x


def _msda_inputs(dtype, shapes_l, P, Lq, seed=0):
    """An msda_case whose value / grad_out are rounded to ``dtype`` (the oracle then sees what the kernel sees) -> (case, tensors)."""
    geo = np.float64 if dtype == F64 else np.float32
    c = msda_case(1234 + seed + P + Lq, 2, 2, 32, Lq, shapes_l, P, geo, loc_range=(-0.3, 1.3))
    value, grad_out = dev(c["value"], dtype), dev(c["grad_out"], dtype)
    c["value"], c["grad_out"] = value.double().cpu().numpy(), grad_out.double().cpu().numpy()
    return c, (value, dev(c["shapes"]), dev(c["level_start"]), dev(c["loc"]), dev(c["attn"]), grad_out)


def _forward_close(dtype, out, ref, what):
    """The bars of tests/test_msda_gpu.py (fp32 / fp64: test_forward_backward_vs_oracle, bf16: test_bf16_storage_...) and of
    tests/test_msda_f16_gpu.py (assert_forward_bound)."""
    out = out.double().cpu().numpy()
    if dtype == F64:
        np.testing.assert_allclose(out, ref, rtol=1e-11, atol=1e-11, err_msg=what)
    elif dtype == F32:
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-5, err_msg=what)
    else:
        half_ulp = 2.0 ** -8 if dtype == BF16 else 2.0 ** -11
        assert np.all(np.abs(out - ref) <= np.abs(ref) * half_ulp + 1e-6), what


def _msda_forward_case(dtype, shapes_l, P, Lq, note="generic"):
    def thunk(guard):
        c, (value, shapes, start, loc, attn, _) = _msda_inputs(dtype, shapes_l, P, Lq)
        out = guard(lambda: alo_hip.msda_forward(value, shapes, start, loc, attn))

        def check():
            ref = O.msda_forward(c["value"], c["shapes"], c["level_start"], c["loc"].astype(np.float64), c["attn"].astype(np.float64))
            _forward_close(dtype, out, ref, "msda_forward")
        return check
    case(f"msda_forward-{note}-{NAMES[dtype]}-L{len(shapes_l)}-P{P}-Lq{Lq}", "alo_msda_forward")(thunk)


def _fused_inputs(dtype, shapes_l, P, Lq, M=2, seed=0):
    L = len(shapes_l)
    g = gen(99 + seed + P + Lq)
    geo = F64 if dtype == F64 else F32
    S = sum(h * w for h, w in shapes_l)
    value = torch.randn(2, S, M, 32, generator=g, device=DEV, dtype=geo).to(dtype)
    offsets = (torch.randn(2, Lq, M, L, P, 2, generator=g, device=DEV, dtype=geo) * 2.5).to(dtype)
    logits = (torch.randn(2, Lq, M, L * P, generator=g, device=DEV, dtype=geo) * 2.0).to(dtype)
    ref = torch.rand(2, Lq, L, 2, generator=g, device=DEV, dtype=geo)
    shapes = torch.tensor(shapes_l, dtype=torch.int32, device=DEV)
    return value, shapes, dev(level_start(shapes_l)), offsets, logits, ref


def _fused_oracle(value, shapes_l, offsets, logits, ref, P):
    from test_msda_f16_gpu import host64, prologue64
    loc, attn = prologue64(offsets, logits, ref, shapes_l, P)
    return O.msda_forward(host64(value), np.asarray(shapes_l, np.int32), level_start(shapes_l), loc, attn)


def _msda_fused_case(dtype, shapes_l, P, Lq):
    def thunk(guard):
        from test_msda_gpu import _prologue_in_torch
        value, shapes, start, offsets, logits, ref = _fused_inputs(dtype, shapes_l, P, Lq)
        fused = guard(lambda: alo_hip.msda_forward_fused(value, shapes, start, offsets, logits, ref))

        def check():
            if dtype == F16:   # tests/test_msda_f16_gpu.py::test_generic_fused_forward_vs_oracle
                _forward_close(F16, fused, _fused_oracle(value, shapes_l, offsets, logits, ref, P), "msda_forward_fused fp16")
                return
            geo = F64 if dtype == F64 else F32   # tests/test_msda_gpu.py::test_fused_prologue_matches_unfused
            loc, attn = _prologue_in_torch(offsets.to(geo), logits.to(geo), ref, shapes, P)
            plain = alo_hip.msda_forward(value, shapes, start, loc, attn, 64)
            if dtype == F64:
                assert (fused - plain).abs().max().item() <= 1e-12
            elif dtype == F32:
                assert (fused - plain).abs().max().item() <= 5e-6
            else:
                assert ((fused.float() - plain.float()).abs() <= plain.float().abs() * 2.0 ** -7 + 1e-6).all()
        return check
    case(f"msda_forward_fused-{NAMES[dtype]}-L{len(shapes_l)}-P{P}-Lq{Lq}", "alo_msda_forward_fused")(thunk)


for _dt in (F32, F64, BF16, F16):
    for _shapes, _p in ((SMALL_L2, 3), (SMALL_L4, 4)):
        _msda_forward_case(_dt, _shapes, _p, 9)
        _msda_fused_case(_dt, _shapes, _p, 9)
_msda_forward_case(BF16, SMALL_L4, 4, 17, note="matrix-pipe")   # msda.hip msda_fwd_bf16_mfma_kernel: 16-query runs, a run of one query


def _merged(offsets, logits):
    """Offsets and logits as column slices of one (N, Lq, 3 M L P) buffer: the `_rows` entry point's strides."""
    N, Lq, M = offsets.shape[:3]
    both = torch.cat([offsets.reshape(N, Lq, -1), logits.reshape(N, Lq, -1)], -1).contiguous()
    off_s, log_s = both[..., :M * 32].view(N, Lq, M, 4, 4, 2), both[..., M * 32:].view(N, Lq, M, 16)
    assert not off_s.is_contiguous() and not log_s.is_contiguous()
    return off_s, log_s


def _msda_hm_case(dtype, merged):
    # msda.hip head-major (wave) kernel: runs of 16 queries per wave: Lq = 17 is a full run and a run of one query
    def thunk(guard):
        value, shapes, start, offsets, logits, ref = _fused_inputs(dtype, SMALL_L4, 4, 17)
        mask = _mask(gen(3), 2, value.shape[1])
        off, log = _merged(offsets, logits) if merged else (offsets, logits)
        vhm = guard(lambda: alo_hip.value_head_major(value, mask))
        got = guard(lambda: alo_hip.msda_forward_fused_hm(vhm, shapes, start, off, log, ref, resident=False))

        def check():   # bf16: tests/test_msda_gpu.py::test_head_major_path_is_bit_identical_and_masks_padding; fp16: assert_forward_bound
            masked = value.masked_fill(mask[..., None, None], 0)
            exact = _fused_oracle(masked, SMALL_L4, offsets, logits, ref, 4)
            if dtype == BF16:
                assert torch.equal(got, alo_hip.msda_forward_fused(masked, shapes, start, offsets, logits, ref))
                assert np.all(np.abs(got.double().cpu().numpy() - exact) <= np.abs(exact) * 2.0 ** -8 + 2e-5)
            else:
                _forward_close(F16, got, exact, "msda_forward_fused_hm fp16")
        return check
    case(f"msda_forward_fused_hm-{NAMES[dtype]}-{'merged-slices' if merged else 'dense'}-Lq17",
         "alo_msda_forward_fused_hm_rows", "alo_value_head_major")(thunk)


for _dt in (BF16, F16):
    for _merged_flag in (False, True):
        _msda_hm_case(_dt, _merged_flag)

RESIDENT_PYRAMID = [(40, 50), (20, 25), (10, 13), (5, 7)]   # the smallest of tests/test_msda_gpu.py's RESIDENT_CASES: levels 2-3 in LDS


def _resident_case(wrong_host_copy):
    # msda.hip msda_fwd_bf16_resident_kernel: Lq = S = 2665: 166 runs of 16 queries and a run of 9; 3 workgroups per (image, head) slab
    def thunk(guard):
        from test_msda_gpu import _prologue_in_torch, _resident_case as inputs
        value, mask, offsets, logits, ref, shapes, start = inputs(2, RESIDENT_PYRAMID, None, 2, 43)
        if wrong_host_copy:   # same total, other levels: "a stale host copy costs time, never correctness"
            shapes._alo_shapes = [(40, 50), (20, 25), (13, 10), (7, 5)]
            assert sum(h * w for h, w in shapes._alo_shapes) == value.shape[1]
        off, log = _merged(offsets, logits)
        vhm = alo_hip.value_head_major(value, mask)
        got = guard(lambda: alo_hip.msda_forward_fused_hm(vhm, shapes, start, off, log, ref, resident="always"))

        def check():   # tests/test_msda_gpu.py::test_resident_forward_is_bit_identical_to_the_plain_head_major_kernel
            shapes._alo_shapes = [tuple(hw) for hw in RESIDENT_PYRAMID]
            assert torch.equal(got, alo_hip.msda_forward_fused_hm(vhm, shapes, start, offsets, logits, ref, resident=False))
            sel = slice(0, None, 7)
            loc, attn = _prologue_in_torch(offsets[:, sel].float(), logits[:, sel].float(), ref[:, sel], shapes, 4)
            exact = O.msda_forward(value.masked_fill(mask[..., None, None], 0).double().cpu().numpy(), shapes.cpu().numpy(),
                                   start.cpu().numpy(), loc.double().cpu().numpy(), attn.double().cpu().numpy())
            assert np.all(np.abs(got[:, sel].double().cpu().numpy() - exact) <= np.abs(exact) * 2.0 ** -8 + 2e-5)
        return check
    case(f"msda_forward_fused_hm-resident-always-{'wrong-host-shapes' if wrong_host_copy else 'merged-slices'}",
         "alo_msda_forward_fused_hm_resident")(thunk)


_resident_case(False)
_resident_case(True)


def _msda_backward_generic_case(dtype):
    def thunk(guard):
        from test_msda_gpu import PER_CORNER, backward_path
        c, (value, shapes, start, loc, attn, grad_out) = _msda_inputs(dtype, SMALL_L2, 3, 9, seed=5)
        assert backward_path(c, dtype) == PER_CORNER
        gv, gl, ga = (t.double().cpu().numpy() for t in guard(lambda: alo_hip.msda_backward(value, shapes, start, loc, attn, grad_out)))

        def check():
            rgv, rgl, rga = O.msda_backward(c["value"], c["shapes"], c["level_start"], c["loc"].astype(np.float64),
                                            c["attn"].astype(np.float64), c["grad_out"])
            scale = max(1.0, np.abs(rgl).max())
            if dtype == F64:     # tests/test_msda_gpu.py::test_forward_backward_vs_oracle
                np.testing.assert_allclose(gv, rgv, rtol=1e-11, atol=1e-11)
                np.testing.assert_allclose(gl, rgl, rtol=1e-10, atol=1e-9)
                np.testing.assert_allclose(ga, rga, rtol=1e-11, atol=1e-11)
            elif dtype == F32:
                np.testing.assert_allclose(gv, rgv, rtol=1e-4, atol=2e-5)
                np.testing.assert_allclose(gl, rgl, rtol=1e-4, atol=2e-5 * scale)
                np.testing.assert_allclose(ga, rga, rtol=1e-4, atol=1e-4)
            elif dtype == BF16:  # tests/test_msda_gpu.py::test_bf16_storage_matches_oracle_on_bf16_rounded_inputs
                np.testing.assert_allclose(gl, rgl, rtol=1e-4, atol=1e-3)
                np.testing.assert_allclose(ga, rga, rtol=1e-4, atol=1e-4)
                np.testing.assert_allclose(gv, rgv, rtol=2.0 ** -7, atol=1e-3)
            else:                # tests/test_msda_f16_gpu.py::test_generic_backward_vs_oracle
                np.testing.assert_allclose(gv, rgv, rtol=2.0 ** -10, atol=2e-5)
                np.testing.assert_allclose(ga, rga, rtol=1e-4, atol=1e-4)
                size = np.asarray(c["shapes"], np.float64)[:, ::-1].reshape(1, 1, 1, 2, 1, 2)
                t = c["loc"].astype(np.float64) * size - 0.5
                smooth = (np.abs(t - np.round(t)) >= 1e-3).all(-1)
                np.testing.assert_allclose(gl[smooth], rgl[smooth], rtol=1e-4, atol=2e-5 * scale)
        return check
    case(f"msda_backward-generic-{NAMES[dtype]}", "alo_msda_backward_hinted")(thunk)


for _dt in (F32, F64, BF16, F16):
    _msda_backward_generic_case(_dt)


@case("msda_backward-tiled-fp32-D32-L4-P4-Lq9", "alo_msda_backward_hinted")
def _(guard):
    # msda.hip msda_bwd_tiled_kernel: 4 x 4 tiles of 16 consecutive queries: Lq = 9 is one ragged run per image
    from test_msda_gpu import TILED, hip_backward
    c = msda_case(1234 + 32 + 9, 2, 2, 32, 9, SMALL_L4, 4, np.float32, loc_range=(-0.3, 1.3))
    gv, gl, ga = (t.double().cpu().numpy() for t in guard(lambda: hip_backward(c, F32, TILED)))   # asserts the route

    def check():   # tests/test_msda_gpu.py::test_forward_backward_vs_oracle, fp32
        rgv, rgl, rga = O.msda_backward(*(c[k].astype(np.float64) if c[k].dtype == np.float32 else c[k]
                                          for k in ("value", "shapes", "level_start", "loc", "attn", "grad_out")))
        np.testing.assert_allclose(gv, rgv, rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(gl, rgl, rtol=1e-4, atol=2e-5 * max(1.0, np.abs(rgl).max()))
        np.testing.assert_allclose(ga, rga, rtol=1e-4, atol=1e-4)
    return check


def _msda_backward_wide_case(dtype):
    # msda_bwd_wide.hip: 16 x 16 query blocks per level: level 0 (17 x 19) is 2 x 2 blocks, three of them ragged; Lq == S = 447
    def thunk(guard):
        from test_msda_bwd_wide_gpu import encoder_case, run_and_check
        shapes_l = [(17, 19), (9, 10), (5, 5), (3, 3)]
        c = encoder_case(shapes_l, 2, 2, np.random.default_rng(5), 3.0, True)
        guard(lambda: run_and_check(c, shapes_l, dtype=dtype))   # the helper asserts the route, calls and checks against the oracle
        return lambda: None
    case(f"msda_backward-wide-{NAMES[dtype]}", "alo_msda_backward_hinted")(thunk)


_msda_backward_wide_case(F32)
_msda_backward_wide_case(BF16)


# ---- correlation -----------------------------------------------------------------------------------------------------------------------
CORR_SHAPES = [(2, 37, 9, 13, 3), (1, 64, 16, 24, 4)]   # (B, C, H, W, levels); 4 levels: the deeper-than-3 chain of alo_corr_build


def _corr_case(B, C, H, W, L):
    # corr.hip: the split pre-pass takes kSplitPx = 64 pixels per workgroup, the contraction kTM = 256 x kTN = 128 tiles of the (HW x HW)
    # volume: HW = 117 is one partial tile each way, HW = 384 is 2 x 3 tiles; C = 37 is no multiple of the 16-channel k-step
    def thunk(guard):
        from alonet.raft.utils.utils import coords_grid
        rng = np.random.default_rng(B * 1000 + C + H)
        f1, f2 = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))
        coords = (coords_grid(B, H, W).numpy() + rng.standard_normal((B, 2, H, W)) * 3.0).astype(np.float32)
        grad_out = dev(rng.standard_normal((B, L * 49, H, W)).astype(np.float32))
        levels = guard(lambda: alo_hip.corr_build(dev(f1), dev(f2), L))
        out = guard(lambda: alo_hip.corr_lookup(levels, dev(coords), 3))
        grads = [torch.randn_like(t) for t in levels]    # read-modify-write: the gradients add to what is there
        grads0 = [t.clone() for t in grads]
        guard(lambda: alo_hip.corr_lookup_backward(grads, dev(coords), grad_out, 3))
        gcoords = guard(lambda: alo_hip.corr_lookup_backward_coords(levels, dev(coords), grad_out, 3))

        def check():   # tests/test_corr_gpu.py::test_build_and_lookup_vs_oracle
            ref_pyr = O.corr_pyramid(f1, f2, L)
            for lvl in range(L):
                np.testing.assert_allclose(levels[lvl].cpu().numpy(), ref_pyr[lvl], rtol=0, atol=3e-5)
            ref = O.corr_lookup([lv.cpu().numpy() for lv in levels], coords, 3)
            np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=1e-5)
            again = alo_hip.corr_lookup_backward([t.clone() for t in grads0], dev(coords), grad_out, 3)   # "plain loads and stores, deterministic"
            for a, b in zip(grads, again):
                same_bits(a, b, "corr_lookup_backward")
            same_bits(gcoords, alo_hip.corr_lookup_backward_coords(levels, dev(coords), grad_out, 3), "corr_lookup_backward_coords")
        return check
    case(f"corr_build+lookup+backward-B{B}-C{C}-{H}x{W}-L{L}", "alo_corr_build", "alo_corr_lookup", "alo_corr_lookup_backward",
         "alo_corr_lookup_backward_coords")(thunk)


def _corr_alt_case(B, C, H, W, L):
    def thunk(guard):
        from alonet.raft.corr import AlternateCorrBlock
        from alonet.raft.utils.utils import coords_grid
        from test_corr_alt_gpu import feature_scale
        rng = np.random.default_rng(B * 7919 + C * 31 + H)
        f1, f2 = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))
        coords = (coords_grid(B, H, W).numpy() + rng.standard_normal((B, 2, H, W)) * 3.0).astype(np.float32)
        got = guard(lambda: AlternateCorrBlock(dev(f1), dev(f2), num_levels=L, radius=3)(dev(coords)))

        def check():   # tests/test_corr_alt_gpu.py::test_against_the_fp32_oracle
            want = O.corr_lookup(O.corr_pyramid(f1, f2, L), coords, 3)
            assert got.shape == want.shape and np.abs(got.cpu().numpy() - want).max() <= 1e-5 * feature_scale(f1, f2)
        return check
    case(f"corr_alt_prepare+lookup-B{B}-C{C}-{H}x{W}-L{L}", "alo_corr_alt_prepare", "alo_corr_alt_lookup")(thunk)


for _shape in CORR_SHAPES:
    _corr_case(*_shape)
    _corr_alt_case(*_shape)


# ---- two-stage glue --------------------------------------------------------------------------------------------------------------------
def _proposals_case(dtype):
    # two_stage.hip: kPropTokens = 512 tokens per block, kFoldTokens = 64; the pyramid of tests/test_two_stage_gpu.py (S = 163: a partial
    # block per image), two images, the second one padded
    def thunk(guard):
        from alonet.deformable_detr.deformable_transformer import encoder_output_proposals
        from test_two_stage_gpu import G19_SHAPES, _mask as pyramid_mask
        mask = pyramid_mask(G19_SHAPES, 2, seed=11).to(DEV)
        memory = torch.randn(2, mask.shape[1], 256, generator=torch.Generator().manual_seed(256)).to(DEV, dtype)
        proposals, keep = guard(lambda: alo_hip.encoder_proposals(mask, G19_SHAPES))
        rows = guard(lambda: alo_hip.mask_rows(memory, keep))
        got_p, got_k, got_m = guard(lambda: alo_hip.encoder_proposals_masked(mask, G19_SHAPES, memory))

        def check():   # tests/test_two_stage_gpu.py::test_encoder_proposals_kernel_vs_torch and ..._masked_kernel_equals_the_two_kernels
            want32, keep32 = encoder_output_proposals(mask, G19_SHAPES)
            want64, keep64 = encoder_output_proposals(mask, G19_SHAPES, dtype=torch.float64)
            assert torch.equal(keep, keep32) and torch.equal(torch.isposinf(proposals), torch.isposinf(want32))
            assert (proposals.double() - want64)[keep64 & keep].abs().max().item() <= 2e-5
            same_bits(rows, memory.masked_fill(~keep.unsqueeze(-1), 0.0), "mask_rows")
            assert torch.equal(got_k, keep)
            same_bits(got_p, proposals, "encoder_proposals_masked: proposals")
            same_bits(got_m, rows, "encoder_proposals_masked: rows")
        return check
    case(f"encoder_proposals+mask_rows+masked-{NAMES[dtype]}", "alo_encoder_proposals", "alo_mask_rows",
         "alo_encoder_proposals_masked")(thunk)


for _dt in (F32, BF16, F16):
    _proposals_case(_dt)


def _queries_case(dtype, K):
    # two_stage.hip alo_proposal_queries: 4 selected proposals per 256-thread block: B K = 2 is half a block, B K = 24 is six blocks
    def thunk(guard):
        from alonet.deformable_detr.deformable_transformer import proposal_pos_embed
        coords = (torch.randn(2, 163, 4, generator=torch.Generator().manual_seed(19)) * 3).to(DEV)
        coords[0, 5], coords[1, 7] = float("inf"), float("-inf")
        topk = torch.randint(0, 163, (2, K), generator=torch.Generator().manual_seed(K))
        topk[:, 0] = torch.tensor([5, 7])
        topk = topk.to(DEV)
        ref, embed = guard(lambda: alo_hip.proposal_queries(coords, topk, dtype))

        def check():
            picked = torch.gather(coords.double(), 1, topk.unsqueeze(-1).expand(-1, -1, 4))
            want = proposal_pos_embed(picked)
            assert (ref.double() - picked.sigmoid()).abs().max().item() <= 1e-6     # tests/test_two_stage_gpu.py
            if dtype == F16:     # tests/test_layers_f16_gpu.py::test_proposal_queries_fp16_vs_the_double_evaluation
                from test_layers_f16_gpu import RND, TINY
                compare(embed, want, RND * want.abs() + TINY, f"proposal_queries fp16 K={K}")
            else:                # tests/test_two_stage_gpu.py::test_proposal_queries_kernel_vs_torch_fp64, bf16: one ulp of the rounded value
                rounded = want.to(BF16).double()
                ulp = 2.0 ** (torch.floor(torch.log2(rounded.abs().clamp_min(2.0 ** -126))) - 7)
                assert ((embed.double() - rounded).abs() <= ulp).all()
        return check
    case(f"proposal_queries-{NAMES[dtype]}-K{K}", "alo_proposal_queries")(thunk)


for _dt in (BF16, F16):
    for _k in (1, 12):
        _queries_case(_dt, _k)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
def _guard_into(seen):
    def guard(fn):
        with GuardedLaunches() as g, torch.no_grad():
            out = fn()
        seen.extend(symbol for symbol, _ in g.seen)
        return out
    return guard


@pytest.mark.parametrize("thunk,expects", CASES)
def test_kernel_stays_in_its_buffers_and_ignores_stale_bytes(thunk, expects):
    seen = []
    check = thunk(_guard_into(seen))
    assert expects <= set(seen), f"not launched: {sorted(expects - set(seen))}"
    assert set(seen) <= set(ROLES)
    check()


# ---- whole models under guard ------------------------------------------------------------------------------------------------------------
def _guarded_model(fn):
    with GuardedLaunches() as g:
        out = fn()
    return out, {symbol for symbol, _ in g.seen}


# The models attach a host copy of the pyramid's shapes, so their fused forward goes through alo_msda_forward_fused_hm_resident (which
# takes the plain head-major kernel by itself at these sizes).
DETR_BF16_LAUNCHES = {
    "alo_stem_conv_pool", "alo_linear_shortk", "alo_linear_packed", "alo_conv1x1_nhwc", "alo_conv3x3_nhwc", "alo_pack_mfma_b",
    "alo_groupnorm_rows", "alo_mask_pyramid", "alo_pos_sine_flat", "alo_encoder_reference_points", "alo_value_proj_head_major",
    "alo_encoder_block", "alo_msda_forward_fused_hm_resident", "alo_add_layernorm", "alo_ffn256"}


def test_deformable_detr_r50_bf16_forward_under_guard(monkeypatch):
    """Two frames of different size, eager (as test_encoder_block_gpu.py::test_graphed_forward_replays_the_fused_loop builds them):
    every launch of the forward under the guard, finite outputs, and the bits of the un-guarded forward."""
    import aloscene
    from alonet.deformable_detr import DeformableDetrR50

    monkeypatch.delenv("ALO_ENC_BLOCK", raising=False)
    torch.manual_seed(0)
    model = DeformableDetrR50(num_classes=91, aux_loss=False, device=torch.device(DEV)).eval().to(BF16)
    cpu = torch.Generator().manual_seed(5)
    fr = [aloscene.Frame(torch.rand(3, 256 - 32 * i, 320, generator=cpu) * 255, normalization="255").norm_resnet() for i in range(2)]
    frames = aloscene.Frame.batch_list(fr).to(DEV).to(BF16)
    with torch.no_grad():
        out, seen = _guarded_model(lambda: model(frames))
        got = {k: out[k].clone() for k in ("pred_logits", "pred_boxes")}
        want = model(frames)
    assert DETR_BF16_LAUNCHES <= seen, sorted(DETR_BF16_LAUNCHES - seen)
    for key, value in got.items():
        assert torch.isfinite(value.float()).all(), key
        assert torch.equal(value, want[key]), key


def test_two_stage_transformer_forward_under_guard(golden):
    from test_two_stage_gpu import _g19_on_gpu
    g, tr, (srcs, masks, poss), L = _g19_on_gpu(golden, BF16)
    with torch.no_grad():
        out, seen = _guarded_model(lambda: tr(srcs, masks, poss, None))
    expected = {"alo_encoder_proposals_masked", "alo_proposal_queries", "alo_msda_forward_fused_hm_resident", "alo_value_proj_head_major",
                "alo_linear_shortk", "alo_add_layernorm", "alo_pack_mfma_b"}
    assert expected <= seen, sorted(expected - seen)
    assert torch.isfinite(out["hs"].float()).all() and torch.isfinite(out["enc_outputs_class"].float()).all()
    assert torch.isfinite(out["init_reference_out"]).all() and not torch.isnan(out["enc_outputs_coord_unact"]).any()


def test_panoptic_head_forward_under_guard():
    import aloscene
    from alonet.deformable_detr_panoptic import DeformableDetrR50Panoptic

    torch.manual_seed(0)
    model = DeformableDetrR50Panoptic(num_classes=250, device=torch.device(DEV)).eval().to(BF16).to(memory_format=torch.channels_last)
    cpu = torch.Generator().manual_seed(9)
    fr = [aloscene.Frame(torch.rand(3, 128 - 32 * i, 160, generator=cpu) * 255, normalization="255").norm_resnet() for i in range(2)]
    frames = aloscene.Frame.batch_list(fr).to(DEV).to(BF16)
    keep = [torch.zeros(300, dtype=torch.bool, device=DEV) for _ in range(2)]
    for k in keep:
        k[torch.arange(3, device=DEV) * 18] = True

    def run():
        out = model(frames, filters=keep)
        return out, model.inference(out, filters=keep)
    with torch.no_grad():
        (out, (boxes, masks)), seen = _guarded_model(run)
    expected = {"alo_groupnorm_rows_act", "alo_conv3x3_small_nhwc", "alo_upsample_add_nhwc", "alo_panoptic_onehot", "alo_conv3x3_nhwc",
                "alo_stem_conv_pool", "alo_encoder_block", "alo_msda_forward_fused_hm_resident"}
    assert expected <= seen, sorted(expected - seen)
    assert out["pred_masks"].shape[:2] == (2, 3) and torch.isfinite(out["pred_masks"].float()).all()
    assert torch.isfinite(out["pred_boxes"].float()).all() and len(masks) == 2 and int(masks[0].as_tensor().sum(0).max()) <= 1


RAFT_LAUNCHES = {"alo_bias_act_nchw", "alo_gru_gate", "alo_gru_update"}


@pytest.mark.parametrize("route", ["default", "alternate-corr", "conv3x3-split"])
def test_raft_fp32_forward_under_guard(golden, monkeypatch, route):
    """G7's frames, 3 iterations.  MIOpen's solver choice varies between runs, so no bits are compared: the per-launch checks are
    the test."""
    from alonet.raft import RAFT, AlternateCorrBlock
    from test_raft_split_route_gpu import KNOB, _g7

    monkeypatch.delenv(KNOB, raising=False)
    if route == "conv3x3-split":
        monkeypatch.setenv(KNOB, "split")
    model = RAFT(corr_block=AlternateCorrBlock).eval() if route == "alternate-corr" else RAFT().eval()
    g, mk = _g7(golden, model)
    model = model.to(DEV)
    f1, f2 = mk(g["img1"], DEV, F32), mk(g["img2"], DEV, F32)
    with torch.no_grad():
        outs, seen = _guarded_model(lambda: model(f1, f2, iters=3))
    expected = RAFT_LAUNCHES | {"default": {"alo_corr_build", "alo_corr_lookup"},
                                "alternate-corr": {"alo_corr_alt_prepare", "alo_corr_alt_lookup"},
                                "conv3x3-split": {"alo_corr_build", "alo_corr_lookup", "alo_conv3x3_nhwc", "alo_pack_mfma_b"}}[route]
    assert expected <= seen, sorted(expected - seen)
    if route != "conv3x3-split":
        assert "alo_conv3x3_nhwc" not in seen
    for o in outs:
        assert torch.isfinite(o["flow"]).all() and torch.isfinite(o["up_flow"]).all()


def test_deformable_transformer_training_step_under_guard():
    """One forward + backward of tests/test_grad_routes_gpu.py's fp32 transformer case, every parameter trainable: the differentiable
    op's forward and the MSDA backward (grad_value: the one output compared at a tolerance, guarded.NONDETERMINISTIC)."""
    from test_grad_routes_gpu import ALL, _t_case
    c = _t_case(F32, False)
    (grads, tags), seen = _guarded_model(lambda: c.hip(ALL, False, True))
    assert {"alo_msda_forward", "alo_msda_backward_hinted"} <= seen, sorted(seen)
    assert sum(n for tag, n in tags.items() if tag.startswith("msda_bwd")) == 4     # the timer sees one record per launch
    live = [g for g in grads.values() if g is not None]
    assert live and all(torch.isfinite(g).all() for g in live)
