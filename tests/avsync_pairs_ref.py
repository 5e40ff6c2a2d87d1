"""float64 restatement of what the reference does with the AVSync classifier beyond scoring aligned rows, for
tests/test_avsync_pairs_cpu.py and tests/test_avsync_pairs_gpu.py:

  * the FC head on every (audio p, video q) pair of a group, on the MATERIALISED concatenation (avsync/models/head.py on the
    repeated rows of sync_contrastive_trainer.py:35-38);
  * the contrastive objective on the (b, k, k) score matrix (sync_contrastive_trainer.py:40-53): audio rows over video columns is
    "av", video columns over audio rows "va", label = the aligned index, logits divided by tau;
  * the shift-accuracy evaluation (scripts/avsync_eval.py:116-167): centre index k // 2, argmax over the k shifted partners, a hit
    within tolerate_range, an example index counted once with its first occurrence.

Also here: the exact-integer head problems, and a torch backend that states the contracts of the three device entry points
(include/avsd.h) with plain torch ops, for the CPU tests."""
import numpy as np
import torch
import torch.nn.functional as F


# ---- the head on a matrix of pairs ----------------------------------------------------------------------------------------------------
def head64(sd, x):
    """sd: state dict of FCHead (fc.0 / fc.3 / fc.6), x (m, 2 D) float64 -> (m, out_dim)"""
    w = {k: v.double() for k, v in sd.items()}
    y = F.relu(F.linear(x, w["fc.0.weight"], w["fc.0.bias"]))
    y = F.relu(F.linear(y, w["fc.3.weight"], w["fc.3.bias"]))
    return F.linear(y, w["fc.6.weight"], w["fc.6.bias"])


def pair_scores64(sd, audio_emb, video_emb):
    """audio_emb (G, P, D), video_emb (G, Q, D) -> (G, P, Q) float64: every pair written out as a row cat(a[g, p], v[g, q])"""
    G, P, D = audio_emb.shape
    Q = video_emb.shape[1]
    rows = torch.empty(G, P, Q, 2 * D, dtype=torch.float64)
    for g in range(G):
        for p in range(P):
            for q in range(Q):
                rows[g, p, q, :D] = audio_emb[g, p].double()
                rows[g, p, q, D:] = video_emb[g, q].double()
    return head64(sd, rows.reshape(-1, 2 * D))[:, 0].reshape(G, P, Q)


def draw_head(dim, seed, out_dim=1):
    """a seeded FCHead state dict whose weights are not symmetric in any sense: N(0, 1 / fan_in) weights, N(0, 0.1^2) biases"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (o, i) in (("fc.0", (dim, 2 * dim)), ("fc.3", (dim // 2, dim)), ("fc.6", (out_dim, dim // 2))):
        sd[name + ".weight"] = torch.randn(o, i, generator=g) / i ** 0.5
        sd[name + ".bias"] = 0.1 * torch.randn(o, generator=g)
    return sd


def draw_embeddings(G, P, Q, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(G, P, D, generator=g).abs(), torch.randn(G, Q, D, generator=g).abs()      # encoder outputs follow a ReLU: >= 0


# ---- exact integers -------------------------------------------------------------------------------------------------------------------
def integer_head(dim, seed, nonzeros=16):
    """W1 in {-1, 0, 1} with `nonzeros` entries per row, W2 and w3 in {-1, 0, 1}, integer biases: with embeddings in {-1, 0, 1}
    |h1| <= nonzeros + 16 = 32, |h2| <= 32 dim + 16, |s| <= (32 dim + 16) dim / 2 + 16 — for dim = 512 below 4.3e6 < 2^24, so every
    partial sum in any order is an exactly representable integer"""
    g = torch.Generator().manual_seed(seed)
    w1 = torch.zeros(dim, 2 * dim)
    for r in range(dim):
        cols = torch.randperm(2 * dim, generator=g)[:nonzeros]
        w1[r, cols] = torch.randint(0, 2, (nonzeros,), generator=g).float() * 2 - 1
    tri = lambda *shape: torch.randint(-1, 2, shape, generator=g).float()  # noqa: E731
    bias = lambda n: torch.randint(-16, 17, (n,), generator=g).float()  # noqa: E731
    return {"fc.0.weight": w1, "fc.0.bias": bias(dim), "fc.3.weight": tri(dim // 2, dim), "fc.3.bias": bias(dim // 2),
            "fc.6.weight": tri(1, dim // 2), "fc.6.bias": bias(1)}


def integer_embeddings(G, P, Q, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (G, P, D), generator=g).float(), torch.randint(-1, 2, (G, Q, D), generator=g).float()


# ---- the contrastive objective ----------------------------------------------------------------------------------------------------------
def first_argmax(x, dim):
    """argmax with a tie going to the lowest index, stated without relying on what torch.argmax does on ties"""
    n = x.shape[dim]
    shape = [1] * x.dim()
    shape[dim] = n
    idx = torch.arange(n).view(shape).expand_as(x)
    return torch.where(x == x.max(dim, keepdim=True).values, idx, torch.full_like(idx, n)).min(dim).values


def contrastive64(scores, tau):
    """scores (b, k, k) with [example, audio, video] -> (av_loss, va_loss, av_acc, va_acc) float64"""
    b, k, k2 = scores.shape
    assert k == k2
    s = scores.double()
    labels = torch.arange(k).repeat(b)
    av = s.reshape(b * k, k)                       # one row per audio, over the videos
    va = s.transpose(1, 2).reshape(b * k, k)       # one row per video, over the audios
    return (F.cross_entropy(av / tau, labels), F.cross_entropy(va / tau, labels),
            (first_argmax(av, 1) == labels).double().mean(), (first_argmax(va, 1) == labels).double().mean())


def line_losses64(scores, tau):
    """scores (G, P, Q) -> (row_loss (G, P) or None, col_loss (G, Q) or None, row_argmax, col_argmax): row p's label is q = p"""
    G, P, Q = scores.shape
    s = scores.double() / tau
    row = col = None
    if P <= Q:
        row = F.cross_entropy(s.reshape(G * P, Q), torch.arange(P).repeat(G), reduction="none").reshape(G, P)
    if Q <= P:
        col = F.cross_entropy(s.transpose(1, 2).reshape(G * Q, P), torch.arange(Q).repeat(G), reduction="none").reshape(G, Q)
    return row, col, first_argmax(scores, 2), first_argmax(scores, 1)


def top2_margin(lines):
    """smallest gap between the largest and the second largest entry over the last axis (inf for lines of one entry)"""
    if lines.shape[-1] < 2:
        return float("inf")
    t = lines.double().topk(2, dim=-1).values
    return float((t[..., 0] - t[..., 1]).min())


# ---- the shift-accuracy evaluation ------------------------------------------------------------------------------------------------------
def shift_eval64(sd_head, audio_emb, video_emb, tolerate_range):
    """embeddings (b, k, D) -> dict(av_scores (b, k), va_scores (b, k), av_pred, va_pred, av_hit, va_hit)"""
    b, k, D = audio_emb.shape
    c = k // 2
    a, v = audio_emb.double(), video_emb.double()
    av = head64(sd_head, torch.cat([a[:, c:c + 1].expand(b, k, D), v], 2).reshape(b * k, 2 * D))[:, 0].reshape(b, k)
    va = head64(sd_head, torch.cat([a, v[:, c:c + 1].expand(b, k, D)], 2).reshape(b * k, 2 * D))[:, 0].reshape(b, k)
    ap, vp = first_argmax(av, 1), first_argmax(va, 1)
    return dict(av_scores=av, va_scores=va, av_pred=ap, va_pred=vp, av_hit=(ap - c).abs() <= tolerate_range, va_hit=(vp - c).abs() <= tolerate_range)


def reduce_unique(indices, av_hits, va_hits):
    """every example index once, with the values of its first occurrence -> (av_acc, va_acc, n)"""
    first = np.unique(np.asarray(indices), return_index=True)[1]
    return float(np.asarray(av_hits, dtype=np.float64)[first].mean()), float(np.asarray(va_hits, dtype=np.float64)[first].mean()), len(first)


# ---- the tiny end-to-end inputs -----------------------------------------------------------------------------------------------------------
def tiny_clips(fixture_audio, b=2, k=3):
    """b examples of k clips: 5 x 96 x 80 gratings (the clip shape of the restatement test in tests/test_avsync_gpu.py) that differ in
    angle, speed, wavelength, brightness and contrast, and mel spectrograms made from fixture["audio"] by rolling it in time, scaling
    and offsetting it.  With the seeded weights of tests/golden/avsync_tiny.pt the scores of two clips lie close together (the biases
    carry most of a score); these inputs were chosen, on the CPU in float64, so that every top-2 margin the tests compare a
    prediction on exceeds 4e-5 (1 + max |s|) several times over (measured: 3.5e-4 against 5.9e-5 for the narrowest line)."""
    from tests import avsync_ref as R

    g = torch.Generator().manual_seed(7)
    vids = torch.stack([torch.stack([R.grating_video_u8(5, 96, 80, 0.4 + 1.3 * i + 0.37 * j, 0.09 - 0.2 * i + 0.11 * j, 11.0 + 14.0 * i + 5.0 * j, 0.5 * i,
                                                        mean=0.3 + 0.2 * ((i + j) % 3), contrast=0.15 + 0.12 * ((2 * i + j) % 3))
                                     for j in range(k)]) for i in range(b)])
    videos = R.normalize_clip(R.u8_to_unit(vids).flatten(0, 1)).view(b, k, 3, 5, 96, 80) + 0.05 * torch.randn(b, k, 3, 5, 96, 80, generator=g)
    n = fixture_audio.shape[0]
    audios = torch.stack([torch.stack([torch.roll(fixture_audio[(i + j) % n], 17 * j + 5 * i, dims=-1) * (1.0 + 0.3 * (j - 1)) + 0.09 * i
                                       for j in range(k)]) for i in range(b)])
    return audios.contiguous(), videos.contiguous()


def tiny_reference(sd, audios, videos):
    """float64 embeddings (b, k, 512) of the restatement tests/avsync_ref.py"""
    from tests import avsync_ref as R

    b, k = audios.shape[:2]
    sd64 = {n: (t.double() if t.is_floating_point() else t) for n, t in sd.items()}
    with torch.no_grad():
        a = R.audio_forward(R._sub(sd64, "audio_encoder."), audios.flatten(0, 1).double()).view(b, k, -1)
        v = R.video_forward(R._sub(sd64, "video_encoder."), videos.flatten(0, 1).double()).view(b, k, -1)
    return a, v


# ---- the contracts of the device entry points in torch ops --------------------------------------------------------------------------------
class TorchBackend:
    """`be=` of asva_amd.avsync for the CPU tests: `conv` on the packed layers (taps (1, 1, 1) only: the head), `half`, `pair_head` and
    `pair_xent` as include/avsd.h states them"""

    @staticmethod
    def conv(x, layer, res=None):
        assert layer.taps == (1, 1, 1) and res is None
        y = F.linear(x.reshape(x.shape[0], -1), layer.w[:, :layer.cin], layer.bias)
        return (y.relu() if layer.relu else y).view(x.shape[0], 1, 1, 1, -1)

    @staticmethod
    def half(x, layer, col, bias):
        return F.linear(x, layer.w[:, col:col + x.shape[1]], bias)

    @staticmethod
    def pair_head(u, vh, l2, l3):
        h1 = (u[:, :, None, :] + vh[:, None, :, :]).relu()                                   # [G, P, Q, H1]
        h2 = (h1 @ l2.w[:, :u.shape[2]].T + l2.bias).relu()
        return h2 @ l3.w[0, :h2.shape[-1]] + l3.bias[0]

    @staticmethod
    def pair_xent(scores, tau):
        G, P, Q = scores.shape
        x = scores * (1.0 / tau)
        r = {"row_argmax": scores.argmax(2).int(), "col_argmax": scores.argmax(1).int()}
        if P <= Q:
            r["row_loss"] = torch.stack([torch.logsumexp(x[:, p], 1) - x[:, p, p] for p in range(P)], 1)
        if Q <= P:
            r["col_loss"] = torch.stack([torch.logsumexp(x[:, :, q], 1) - x[:, q, q] for q in range(Q)], 1)
        if P == Q:
            lab = torch.arange(P)
            r.update(av_loss=r["row_loss"].mean(), va_loss=r["col_loss"].mean(), av_acc=(r["row_argmax"] == lab).float().mean(),
                     va_acc=(r["col_argmax"] == lab).float().mean())
        return r
