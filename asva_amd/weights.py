"""Weight packing: reference state_dict tensors -> the layouts the gfx950 kernels read.

All GEMM-class weights become bf16 [N][K] matrices (K contiguous):
  * nn.Linear weight [out, in]                      -> as is
  * 1x1 nn.Conv2d weight [out, in, 1, 1]            -> [out, in]
  * 3x3 nn.Conv2d weight [out, in, 3, 3]            -> [out, 9*cin_pad], k = (kh*3 + kw)*cin_pad + c
    (cin padded to a multiple of 8 with zeros: conv_in has 4 input channels)
  * GEGLU proj weight [2*Nh, K] (diffusers: value rows then gate rows) -> per 32-row block
    [16 value rows | 16 gate rows] so one MFMA accumulator fragment holds value and gate of the
    same output feature in the same lane (see gemm.hip epilogue)
  * output rows are padded to a multiple of 4 where the layer has fewer (conv_out: 4 -> 4 ok).
Biases and norm parameters stay f32.
"""
from __future__ import annotations

import torch

from . import precision as P


def to_act(w: torch.Tensor) -> torch.Tensor:
    """f32 values -> the 16-bit storage type.  In split-precision mode (precision.SPLIT) the result is the main plane of a
    twin allocation [2, ...]: plane 0 = round16(w), plane 1 = round16(w - plane 0); the rest plane travels with every view
    of the result (same offset in the second half of the storage)."""
    w = w.detach().float().contiguous()
    if not P.SPLIT or w.device.type == "meta":
        return w.to(P.ACT)
    n = w.numel()
    npad = (n + 7) // 8 * 8
    base = torch.zeros((2, npad), dtype=P.ACT, device=w.device)
    main = w.reshape(-1).to(P.ACT)
    base[0, :n] = main
    base[1, :n] = (w.reshape(-1) - main.float()).to(P.ACT)
    return base[0, :n].view(w.shape)


def to_planes(w: torch.Tensor):
    """f32 values -> (main, rest) as two separate 16-bit tensors, whatever the process-wide mode: the weights of a three-pass
    product under the per-layer precision plan (precision.py)"""
    w = w.detach().float().contiguous()
    main = w.to(P.ACT)
    if w.device.type == "meta":
        return main, torch.empty_like(main)
    return main, (w - main.float()).to(P.ACT)


def is_twin(t: torch.Tensor) -> bool:
    """True for a view into the first half of a twin allocation (see to_act)"""
    nb = t.untyped_storage().nbytes()
    if t.numel() == 0 or nb % 32:
        return False
    last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return (t.storage_offset() + last + 1) * t.element_size() <= nb // 2


def rest_of(t: torch.Tensor) -> torch.Tensor:
    """the rest plane of a twin tensor, as a view with the same shape and strides"""
    half = t.untyped_storage().nbytes() // 2 // t.element_size()
    return torch.as_strided(t, t.shape, t.stride(), t.storage_offset() + half)


def from_act(t: torch.Tensor) -> torch.Tensor:
    """the f32 values a kernel reconstructs from a packed 16-bit tensor (main + rest in split mode)"""
    if P.SPLIT and is_twin(t):
        return t.float() + rest_of(t).float()
    return t.float()


def pack_linear(w: torch.Tensor) -> torch.Tensor:
    return to_act(w)


def pack_conv1x1(w: torch.Tensor) -> torch.Tensor:
    return to_act(w.detach().reshape(w.shape[0], w.shape[1]))


def pack_conv3x3(w: torch.Tensor, cin_pad: int | None = None, cout_pad: int | None = None) -> torch.Tensor:
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3
    cin_pad = cin_pad or (cin + 7) // 8 * 8
    cout_pad = cout_pad or (cout + 3) // 4 * 4
    p = torch.zeros((cout_pad, 3, 3, cin_pad), dtype=torch.float32, device=w.device)
    p[:cout, :, :, :cin] = w.detach().float().permute(0, 2, 3, 1)
    return to_act(p.reshape(cout_pad, 9 * cin_pad))


def subpixel_conv3x3(wf: torch.Tensor) -> torch.Tensor:
    """3x3 pad-1 convolution behind a nearest 2x upsample (FFSpatioTempResUpsample3D, ff_spatio_temp_resnet_3d.py:48-55) as FOUR 2x2
    convolutions on the ORIGINAL image, one per output-pixel parity (dy, dx): output pixel (2y + dy, 2x + dx) of the upsampled
    convolution sees input rows y + dy - 1 and y + dy (columns likewise), because upsampled row 2y + dy + ky - 1 is input row
    y + ((dy + ky - 1) >> 1) — so the 3 kernel rows fold onto 2 input rows with summed weights: dy = 0: {w0 | w1 + w2}, dy = 1:
    {w0 + w1 | w2}.  Exactly the same function (the sums are formed in f32 before the one rounding to storage), 4/9 of the multiplies.
    wf [cout, 3, 3, cin] f32 (kernel layout, channels last) -> [4 * cout, 2 * 2 * cin]: row (2 dy + dx) * cout + co, column
    (2 i + j) * cin + ci = the weight of input pixel (y + dy - 1 + i, x + dx - 1 + j) (AVSD_GEMM_CONV3 with ups = 2, include/avsd.h)."""
    cout, kh, kw, cin = wf.shape
    assert kh == 3 and kw == 3
    sets = (((0,), (1, 2)), ((0, 1), (2,)))            # sets[d][i]: kernel rows (columns) that land on input row (column) offset d - 1 + i
    out = torch.zeros((2, 2, cout, 2, 2, cin), dtype=torch.float32, device=wf.device)
    for dy in range(2):
        for dx in range(2):
            for i in range(2):
                for j in range(2):
                    for ky in sets[dy][i]:
                        for kx in sets[dx][j]:
                            out[dy, dx, :, i, j, :] += wf[:, ky, kx, :]
    return out.reshape(4 * cout, 4 * cin)


def subpixel_ups(wf: torch.Tensor, b: torch.Tensor):
    """an upsampler's 3x3 convolution and bias in the sub-pixel form: wf [cout, 3, 3, cin] f32, b [cout] -> the [4 cout, 4 cin] matrix
    of subpixel_conv3x3 and the bias once per output-pixel parity.  Padding and the kernel's layout rule (whole 64-channel K tiles per
    tap, whole column tiles per parity) are the caller's: the UNet tests its padded channel counts, the VAE the checkpoint's"""
    return subpixel_conv3x3(wf), b.repeat(4)


def geglu_row_order(nh: int) -> torch.Tensor:
    """Packed row r of a GEGLU projection with nh output features reads source row order[r]."""
    assert nh % 16 == 0, "GEGLU packing needs the inner dim to be a multiple of 16"
    blk = torch.arange(nh // 16).repeat_interleave(32)
    p = torch.arange(32).repeat(nh // 16)
    return torch.where(p < 16, blk * 16 + p, nh + blk * 16 + p - 16)


def pack_geglu(w: torch.Tensor, b: torch.Tensor | None):
    nh = w.shape[0] // 2
    order = geglu_row_order(nh).to(w.device)
    wp = to_act(w.detach()[order])
    bp = None if b is None else b.detach()[order].float().contiguous()
    return wp, bp


def pack_frag(wp: torch.Tensor) -> torch.Tensor:
    """packed 16-bit weights [N, K] -> MFMA-fragment order [N / 32, K / 16, 64, 8] (AVSD_GEMM_W_FRAG, include/avsd.h): element
    (f, s, l, e) = W[32 f + (l & 31)][16 s + 8 (l >> 5) + e] — what lane l of a wave feeds the 32x32x16 MFMA of k-step s for the
    32 columns of fragment f; one k-step of one fragment is 1 KB, contiguous (csrc/nstream.hip streams it straight into registers)"""
    N, K = wp.shape
    assert N % 32 == 0 and K % 16 == 0
    return wp.reshape(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(N // 32, K // 16, 64, 8)


def group_qkv(t: torch.Tensor, heads: int = 8) -> torch.Tensor:
    """rows [q | k | v] of a fused projection (dim 0 = 3 C: a weight [3 C, K], its column sums or bias [3 C]) regrouped for the
    one-launch temporal attention (csrc/tblock.hip): 4 groups of heads / 4 heads, each [q | k | v] of its heads (3 C / 4 rows)
    padded with zeros to the next multiple of 32 + 16 — at C = 320: 240 -> 256 rows, [1024, ...] in all"""
    C = t.shape[0] // 3
    assert t.shape[0] == 3 * C and heads % 4 == 0 and C % heads == 0
    n = C // 4                                # rows of q (or k, or v) per group
    pad = (3 * n + 31) // 32 * 32
    out = torch.zeros((4, pad) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    src = t.reshape(3, 4, n, *t.shape[1:])
    for j in range(3):
        out[:, j * n:(j + 1) * n] = src[j]
    return out.reshape(4 * pad, *t.shape[1:])


def pad_rows(w: torch.Tensor, mult: int = 4) -> torch.Tensor:
    n = w.shape[0]
    if n % mult == 0:
        return w
    pad = torch.zeros((mult - n % mult,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
    return torch.cat([w, pad], 0).contiguous()


# ---- the packed blob -------------------------------------------------------------------------------------------------------------
class _Pk:
    """attribute bag of device tensors (views into the packed blob)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Ref:
    """placeholder for item `idx` of the packed blob until the blob exists"""

    def __init__(self, idx: int):
        self.idx = idx


class Blob:
    """Kernel-layout tensors of one model, collected by `reg` and laid out in ONE 256-byte-aligned device blob by `finish`: the unit
    the multi-GPU start-up broadcasts (asva_amd.dist) and the launch-plan export ships as a CONST region (asva_amd.plan)."""

    def __init__(self):
        self.items = []        # packed tensors, on the parameters' device (or meta: layout only)

    def reg(self, t: torch.Tensor) -> _Ref:
        self.items.append(t.contiguous())
        return _Ref(len(self.items) - 1)

    def reg_tree(self, root):
        """`reg` for every tensor in a tree of attribute bags and lists, in attribute order (the order of the blob's items); -> root"""
        if isinstance(root, _Pk):
            for k, v in list(root.__dict__.items()):
                root.__dict__[k] = self.reg(v) if isinstance(v, torch.Tensor) else self.reg_tree(v)
        elif isinstance(root, list):
            for v in root:
                self.reg_tree(v)
        return root

    def finish(self, root: _Pk, device, meta: bool = False) -> _Pk:
        """lays all items out in one blob on `device`, replaces the placeholders inside `root` by typed views of it and stamps
        `root` with the blob and the precision.pack_key() it was packed under"""
        offs, total = [], 0
        for t in self.items:
            offs.append(total)
            total += (t.numel() * t.element_size() + 255) // 256 * 256
        # split precision: the blob is a twin allocation like every split tensor — the rest plane of item i sits at the
        # same offset in the second half, so every view below carries it along (precision.py)
        blob = torch.zeros(total * (2 if P.SPLIT else 1), dtype=torch.uint8, device=device)
        views = []
        for t, o in zip(self.items, offs):
            nb = t.numel() * t.element_size()
            if not meta:   # meta parameters: layout only — the bytes arrive by broadcast (asva_amd.dist)
                blob[o:o + nb].copy_(t.reshape(-1).view(torch.uint8))
                if P.SPLIT and t.dtype == P.ACT:
                    if not is_twin(t):
                        raise RuntimeError("split-precision packing: a 16-bit item was not produced by weights.to_act")
                    blob[total + o:total + o + nb].copy_(rest_of(t).reshape(-1).view(torch.uint8))
            views.append(blob[o:o + nb].view(t.dtype).view(t.shape))

        def resolve(obj):
            if isinstance(obj, _Pk):
                for k, v in list(obj.__dict__.items()):
                    if isinstance(v, _Ref):
                        obj.__dict__[k] = views[v.idx]
                    else:
                        resolve(v)
            elif isinstance(obj, list):
                for v in obj:
                    resolve(v)

        resolve(root)
        root.blob = blob
        root.key = P.pack_key()
        root.split = P.SPLIT
        return root


def pack_device(device, own=None, ops=None, who="pack"):
    """pack()'s device argument, normalised for its cache test: "cuda" is the current device, None (any device) stays None.  Called again
    with the model's `own` device (it stands in for None) and kernel module once pack() has to pack: the kernels must be able to
    read the result (ops.EMULATED: tests/emu_ops.py seam)."""
    if device is not None:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
    if own is None:
        return device
    device = own if device is None else device
    if device.type == "meta":
        raise RuntimeError(f"{who}: pass the target device explicitly for a meta-initialised model")
    if device.type != "cuda" and not getattr(ops, "EMULATED", False):
        raise RuntimeError(f"{who}: the MI355X path needs a cuda (HIP) device; move the model with .to('cuda') first — "
                           "there is no CPU compute path")
    return device
