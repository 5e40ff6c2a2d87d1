"""Whole-track animation on the MI355X (-m gpu): the turnover kernel bit-exact against torch inside poisoned memory, and
AudioCondAnimationPipeline.animate_track against what it is defined to be - window 0 a single-clip `__call__`, the chain a sequence
of explicit `__call__`s handing over the last frame - on the tiny UNet / VAE (F = 4: a hop of 3 frames), bit for bit.

Why the bounds are 0: chain and by-hand form issue the same kernels on the same inputs in the same order, the tile choice is
static (tests/test_determinism_gpu.py), and no kernel on the path has atomics."""
import pytest
import torch

from tests.helpers import filled_unet, load_golden
from tests.test_host_cpu import TINY_VAE, _filled_vae

pytestmark = pytest.mark.gpu

STEPS = 3
SEED = 11


# ---- avsd_window_turnover --------------------------------------------------------------------------------------------------
def _poisoned(shape, gen, pad=37):
    """a tensor of `shape` in the middle of a NaN-filled allocation -> (view, whole buffer, offset)"""
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    view = buf[pad:pad + n].view(shape)
    view.copy_(torch.randn(shape, generator=gen).cuda())
    return view, buf, pad


def _untouched(buf, pad, n):
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all())


@pytest.mark.parametrize("shape", [(1, 4, 2, 1, 1), (2, 4, 4, 3, 5), (1, 4, 12, 8, 8), (1, 3, 1, 2, 3), (2, 2, 3, 4, 4)])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("sigma", [1.0, 0.7310585975646973])
def test_window_turnover_is_bit_exact(shape, in_place, sigma):
    from asva_amd import ops

    B, C, F, H, W = shape
    gen = torch.Generator().manual_seed(B * 1000 + F * 10 + H)
    x_prev, pbuf, ppad = _poisoned(shape, gen)                       # offsets of 37 floats: rows are 4-byte aligned only
    noise, nbuf, npad = _poisoned((B, C, F - 1, H, W), gen, pad=5)
    x_next, obuf, opad = (x_prev, pbuf, ppad) if in_place else _poisoned(shape, gen, pad=3)
    prev0, noise0 = x_prev.clone(), noise.clone()
    want = torch.cat([prev0[:, :, F - 1:], noise0 * sigma], dim=2)
    got = ops.window_turnover(x_prev, noise, x_next if not in_place else None, sigma)
    torch.cuda.synchronize()
    assert got.data_ptr() == x_next.data_ptr()
    assert torch.equal(x_next.view(torch.int32), want.view(torch.int32))             # bits, not values: -0.0 and NaN payloads count
    assert torch.equal(noise, noise0) and (in_place or torch.equal(x_prev, prev0))   # inputs are read only
    n = x_prev.numel()
    assert _untouched(pbuf, ppad, n) and _untouched(nbuf, npad, noise.numel()) and _untouched(obuf, opad, n)


def test_window_turnover_refuses_overlaps_and_bad_shapes():
    from asva_amd import _lib, ops

    buf = torch.zeros(4 * 4 * 16 * 2, device="cuda")
    x = buf[:256].view(1, 4, 4, 4, 4)
    noise = torch.zeros(1, 4, 3, 4, 4, device="cuda")
    with pytest.raises(ValueError, match="not overlap"):
        ops.window_turnover(x, noise, buf[16:272].view(1, 4, 4, 4, 4))
    with pytest.raises(ValueError, match="noise must not overlap"):
        ops.window_turnover(x, buf[64:256].view(1, 4, 3, 4, 4), x)
    with pytest.raises(ValueError, match="noise must be"):
        ops.window_turnover(x, noise[:, :, :2].contiguous(), x)
    # the entry point itself refuses them too (a host without this binding)
    h = _lib.lib()
    assert h.avsd_window_turnover(x.data_ptr(), noise.data_ptr(), x.data_ptr() + 64, 1.0, 1, 4, 4, 16, None) == -1
    assert b"overlap" in h.avsd_last_error()
    assert h.avsd_window_turnover(x.data_ptr(), x.data_ptr() + 256, x.data_ptr(), 1.0, 1, 4, 4, 16, None) == -1
    assert h.avsd_window_turnover(x.data_ptr(), None, x.data_ptr(), 1.0, 1, 4, 4, 16, None) == -1
    assert h.avsd_window_turnover(x.data_ptr(), noise.data_ptr(), x.data_ptr(), 1.0, 1, 4, 0, 16, None) == -1


# ---- animate_track ------------------------------------------------------------------------------------------------------------
class _Tiny:
    """one tiny pipeline per scheduler, and the inputs of a 3-window track, built once per module"""

    def __init__(self):
        self.g = g = load_golden("unet_tiny_e2e.pt")
        self.f, self.h, self.w = g["sample"].shape[2:]
        assert (self.f, self.h, self.w) == (4, 8, 8)
        gen = torch.Generator().manual_seed(3)
        self.il = torch.randn(1, 4, self.h, self.w, generator=gen) * 0.18215
        d = g["audio"].shape[-1]
        self.audio = torch.randn(4, 229, d, generator=gen)                  # four distinct windows' worth of conditioning rows
        self.null = g["audio"][:1]
        self.pipes = {}

    def pipe(self, kind):
        from asva_amd.pipeline import AudioCondAnimationPipeline
        from asva_amd.schedulers import PNDMScheduler, UniPCMultistepScheduler

        if kind not in self.pipes:
            sched = PNDMScheduler() if kind == "pndm" else UniPCMultistepScheduler()
            p = AudioCondAnimationPipeline(unet=filled_unet(self.g["config"]), scheduler=sched, vae=_filled_vae(TINY_VAE))
            p.to("cuda")
            p.set_progress_bar_config(disable=True)
            self.pipes[kind] = p
        return self.pipes[kind]

    def common(self):
        return dict(texts=[""], text_encodings=[self.g["text"][:1]], height=self.h * 8, width=self.w * 8, num_inference_steps=STEPS,
                    audio_guidance_scale=4.0, null_audio_encodings=self.null, audio_masks=self.g["mask"])

    def track(self, kind, n_windows=3, **kw):
        gen = torch.Generator(device="cuda").manual_seed(SEED)
        args = dict(self.common(), image_latents=self.il, audio_encodings=self.audio[:n_windows], video_length=self.f, generator=gen,
                    output_type="uint8_device")
        args.update(kw)
        return self.pipe(kind).animate_track(**args)

    def noises(self, n):
        """the draws animate_track makes from its generator, in order"""
        gen = torch.Generator(device="cuda").manual_seed(SEED)
        return [torch.randn(1, 4, self.f - 1, self.h, self.w, generator=gen, device="cuda") for _ in range(n)]


@pytest.fixture(scope="module")
def tiny():
    return _Tiny()


@pytest.fixture(scope="module")
def latent_track(tiny):
    """the 3-window PNDM track with latent hand-over, computed once and only read by the tests that share it"""
    return tiny.track("pndm")


@pytest.mark.parametrize("kind", ["pndm", "unipc"])
def test_window_0_is_the_single_clip_call(tiny, kind):
    F = tiny.f
    frames = tiny.track(kind, n_windows=2)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    clip = tiny.pipe(kind)(**tiny.common(), video_length=F, image_latents=tiny.il, audio_encodings=tiny.audio[:1], generator=gen,
                           output_type="uint8_device", return_dict=False)
    assert frames.shape == (1 + 2 * (F - 1), tiny.h * 8, tiny.w * 8, 3) and frames.dtype == torch.uint8
    assert torch.equal(frames[:F], clip[0])
    assert not torch.equal(frames[F:2 * F - 1], clip[0][1:])                  # ... and window 1 is not window 0 again


def _by_hand(tiny, kind, handover, n_windows=3):
    """the chain written out: one `__call__` per window, handing over the last frame, each decoded"""
    pipe, F = tiny.pipe(kind), tiny.f
    lat0, pieces = tiny.il, []
    for k, noise in enumerate(tiny.noises(n_windows)):
        lat = pipe(**tiny.common(), video_length=F, image_latents=lat0, audio_encodings=tiny.audio[k:k + 1], noise=noise,
                   output_latents=True)
        frames = pipe.vae.decode_to_uint8_frames(lat)[0]
        pieces.append(frames if k == 0 else frames[1:])
        if handover == "latent":
            lat0 = lat[:, :, F - 1]
        else:
            img = (frames[F - 1].permute(2, 0, 1)[None].float() / 255.0) * 2.0 - 1.0
            lat0 = pipe.vae.encode(img).latent_dist.mode() * pipe.vae.config.scaling_factor
    return torch.cat(pieces)


def test_latent_chain_equals_three_explicit_calls(tiny, latent_track):
    want = _by_hand(tiny, "pndm", "latent")
    assert latent_track.shape == want.shape == (10, 64, 64, 3)
    assert int((latent_track != want).sum()) == 0


def test_latent_chain_equals_three_explicit_calls_unipc(tiny):
    assert torch.equal(tiny.track("unipc"), _by_hand(tiny, "unipc", "latent"))


def test_pixel_chain_equals_its_by_hand_form(tiny, latent_track):
    got = tiny.track("pndm", handover="pixel")
    assert torch.equal(got, _by_hand(tiny, "pndm", "pixel"))
    F = tiny.f
    assert torch.equal(got[:F], latent_track[:F]) and not torch.equal(got[F:], latent_track[F:])    # the VAE round trip is not free


def test_seam_frames_appear_once_and_come_from_one_latent(tiny, latent_track):
    from asva_amd.data_utils import track_windows

    pipe, F = tiny.pipe("pndm"), tiny.f
    # each window decoded whole: frame F-1 of window k-1 and frame 0 of window k hold the same latent
    lat0, lats = tiny.il, []
    for k, noise in enumerate(tiny.noises(3)):
        lats.append(pipe(**tiny.common(), video_length=F, image_latents=lat0, audio_encodings=tiny.audio[k:k + 1], noise=noise,
                         output_latents=True))
        lat0 = lats[-1][:, :, F - 1]
    for a, b in zip(lats, lats[1:]):
        assert torch.equal(a[:, :, F - 1].view(torch.int32), b[:, :, 0].view(torch.int32))
    # the output holds the seam once: 1 + W (F - 1) frames, and what track_windows says for a track that long
    win, fps = F * 16000 // 6, 6
    n_samples = 2 * ((F - 1) * 16000 // fps) + win                  # fills window 2: nothing to trim
    _, W, n_frames, _ = track_windows(n_samples, 16000, fps, F)
    assert W == 3 and n_frames == latent_track.shape[0] == 1 + 3 * (F - 1)
    cut = tiny.track("pndm", n_samples=n_samples)
    assert cut.shape[0] == n_frames <= latent_track.shape[0] and torch.equal(cut, latent_track[:n_frames])
    shorter = 2 * ((F - 1) * 16000 // fps) + win - 2 * 16000 // fps + 1
    n_short = track_windows(shorter, 16000, fps, F)[2]
    assert F <= n_short < n_frames and torch.equal(tiny.track("pndm", n_samples=shorter), latent_track[:n_short])
    with pytest.raises(ValueError, match="windows"):
        tiny.track("pndm", n_samples=16000)


def test_audio_reaches_its_window(tiny, latent_track):
    F = tiny.f
    swapped = tiny.track("pndm", audio_encodings=tiny.audio[[0, 2, 1]])
    assert torch.equal(swapped[:F], latent_track[:F])                         # window 0: same audio, same frames
    for k in (1, 2):                                                          # from the first changed window on, every window differs
        a, b = F + (k - 1) * (F - 1), F + k * (F - 1)
        assert not torch.equal(swapped[a:b], latent_track[a:b])
    last = tiny.track("pndm", audio_encodings=tiny.audio[[0, 1, 3]])
    assert torch.equal(last[:2 * F - 1], latent_track[:2 * F - 1]) and not torch.equal(last[2 * F - 1:], latent_track[2 * F - 1:])


def test_one_graph_serves_every_window_and_the_next_track(tiny, latent_track):
    from asva_amd.pipeline import AudioCondAnimationPipeline
    from asva_amd.schedulers import PNDMScheduler

    pipe = AudioCondAnimationPipeline(unet=filled_unet(tiny.g["config"]), scheduler=PNDMScheduler(), vae=_filled_vae(TINY_VAE))
    pipe.to("cuda")
    pipe.set_progress_bar_config(disable=True)
    kw = dict(tiny.common(), image_latents=tiny.il, audio_encodings=tiny.audio[:3], video_length=tiny.f, output_type="uint8_device")
    first = pipe.animate_track(**kw, generator=torch.Generator(device="cuda").manual_seed(SEED))
    assert pipe._engine.use_graph and pipe._engine.captures == 1
    again = pipe.animate_track(**dict(kw, audio_encodings=tiny.audio[1:4]), generator=torch.Generator(device="cuda").manual_seed(SEED))
    assert pipe._engine.captures == 1
    assert torch.equal(first, latent_track) and not torch.equal(again, first)      # a fresh pipeline gives the shared track's bits


def test_output_type_and_on_window(tiny, latent_track):
    F, seen = tiny.f, []
    host = tiny.track("pndm", output_type="uint8", on_window=lambda k, fr: seen.append((k, fr)))
    assert latent_track.is_cuda and not host.is_cuda and torch.equal(host, latent_track.cpu())
    assert [k for k, _ in seen] == [0, 1, 2] and [fr.shape[0] for _, fr in seen] == [F, F - 1, F - 1]
    assert all(not fr.is_cuda for _, fr in seen) and torch.equal(torch.cat([fr for _, fr in seen]), host)
    seen.clear()
    tiny.track("pndm", n_windows=2, on_window=lambda k, fr: seen.append((k, fr)))
    assert [k for k, _ in seen] == [0, 1] and all(fr.is_cuda for _, fr in seen)


def test_batched_tracks_and_bad_modes_are_refused(tiny):
    with pytest.raises(ValueError, match="one track at a time"):
        tiny.track("pndm", image_latents=torch.cat([tiny.il, tiny.il]))
    with pytest.raises(ValueError, match="handover"):
        tiny.track("pndm", handover="jpeg")
    with pytest.raises(ValueError, match="output_type"):
        tiny.track("pndm", output_type="float")


def test_waveform_track_slices_the_audio_on_the_device(tiny):
    """with a waveform the windows are cut on the device at track_windows' starts and encoded in batches of at most 16: a stand-in
    encoder that returns each window's first samples shows which samples every window heard"""
    from asva_amd.data_utils import track_windows

    pipe, F = tiny.pipe("pndm"), tiny.f
    d = tiny.g["audio"].shape[-1]
    calls = []

    class Proc:
        def __call__(self, audios, device=None):
            calls.append(len(audios))
            assert all(a.is_cuda and a.shape == (1, F * 16000 // 6) for a in audios)
            return torch.stack([a[0, :229, None].expand(229, d) for a in audios])[:, None]         # token t = sample t of the window

    class Enc:
        def __call__(self, mel, normalize=False, return_dict=False):
            return None, mel[:, 0], None

    n = F * 16000 // 6 + 16 * ((F - 1) * 16000 // 6) + 100                       # 18 windows: a batch of 16 and one of 2
    windows, W, n_frames, _ = track_windows(n, 16000, 6, F)
    assert W == 18
    wave = torch.randn(1, n, generator=torch.Generator().manual_seed(5)) * 0.05
    old = pipe.audio_processor, pipe.audio_encoder, pipe.melspectrogram_shape
    pipe.audio_processor, pipe.audio_encoder, pipe.melspectrogram_shape = Proc(), Enc(), (229, d)
    heard = []
    real = pipe.unet.set_conditioning
    pipe.unet.set_conditioning = lambda text, audio, masks, fr: (heard.append(audio.clone()), real(text, audio, masks, fr))[1]
    try:
        frames = pipe.animate_track(None, wave, image_latents=tiny.il, texts=[""], text_encodings=[tiny.g["text"][:1]], video_length=F,
                                    height=64, width=64, num_inference_steps=2, audio_guidance_scale=4.0, audio_masks=tiny.g["mask"],
                                    generator=torch.Generator(device="cuda").manual_seed(SEED), output_type="uint8_device")
    finally:
        pipe.audio_processor, pipe.audio_encoder, pipe.melspectrogram_shape = old
        del pipe.unet.set_conditioning
    assert frames.shape[0] == n_frames and len(heard) == W
    assert calls == [16, 2]
    padded = torch.cat([wave[0], torch.zeros(windows[-1][0] + F * 16000 // 6 - n)])
    for (s, _), a in zip(windows, heard):
        assert a.shape == (2, 229, d) and bool((a[0] == 0).all())                 # [null, audio]: the null row is the all-zero mel
        assert torch.equal(a[1, :, 0].cpu(), padded[s:s + 229]) and torch.equal(a[1, :, -1].cpu(), padded[s:s + 229])


# ---- the writer with the device encoder, and the driver -----------------------------------------------------------------------
def test_writer_appends_device_encoded_frames(tmp_path):
    from asva_amd.video_io import MjpegAviWriter, encode_jpeg_frames, read_mjpeg_avi, walk_mjpeg_avi

    gen = torch.Generator().manual_seed(9)
    pieces = [torch.randint(0, 256, (n, 16, 24, 3), generator=gen, dtype=torch.uint8).cuda() for n in (4, 3)]
    path = str(tmp_path / "dev.avi")
    w = MjpegAviWriter(path, 6, (16, 24), 16000, encoder="device")
    assert [w.append(p) for p in pieces] == [4, 7]
    w.close(torch.zeros(1, 7 * 16000 // 6))
    jpegs = walk_mjpeg_avi(path)[0]
    assert jpegs == encode_jpeg_frames(pieces[0]) + encode_jpeg_frames(pieces[1])          # the device encoder's streams, piece by piece
    video, fps, audio, _ = read_mjpeg_avi(path, decoder="host")
    assert video.shape == (7, 16, 24, 3) and fps == 6.0 and audio.shape == (1, 7 * 16000 // 6)


def test_generate_track_writes_one_file_as_long_as_the_audio(tiny, tmp_path):
    import numpy as np
    from PIL import Image
    from scipy.io import wavfile

    from asva_amd.data_utils import track_windows
    from asva_amd.pipeline import generate_track
    from asva_amd.video_io import read_mjpeg_avi

    pipe, F = tiny.pipe("pndm"), tiny.f
    d = tiny.g["audio"].shape[-1]

    class Proc:
        def __call__(self, audios, device=None):
            return torch.stack([a[0, :229, None].expand(229, d) for a in audios])[:, None]

    class Enc:
        def __call__(self, mel, normalize=False, return_dict=False):
            return None, mel[:, 0], None

    rng = np.random.default_rng(4)
    n = 22050 * 3 // 2                                                              # 1.5 s at 22.05 kHz -> 24000 samples at 16 kHz
    wavfile.write(str(tmp_path / "a.wav"), 22050, (rng.uniform(-0.5, 0.5, n) * 32767).astype(np.int16))
    Image.fromarray(rng.integers(0, 256, (80, 100, 3), dtype=np.uint8)).save(str(tmp_path / "i.png"))
    _, W, n_frames, _ = track_windows(24000, 16000, 6, F)
    assert (W, n_frames) == (3, 9)
    old = pipe.audio_processor, pipe.audio_encoder, pipe.melspectrogram_shape
    pipe.audio_processor, pipe.audio_encoder, pipe.melspectrogram_shape, pipe.generation_steps = Proc(), Enc(), (229, d), 2
    try:
        kw = dict(image_path=str(tmp_path / "i.png"), audio_path=str(tmp_path / "a.wav"), category_text_encoding=tiny.g["text"][:1],
                  image_size=(64, 64), video_num_frame=F, seed=1, device=torch.device("cuda"))
        frames, audio = generate_track(pipe, **kw)
        with pytest.warns(RuntimeWarning, match="Motion-JPEG"):
            path = generate_track(pipe, **kw, save_path=str(tmp_path / "out" / "track.mp4"))
    finally:
        pipe.audio_processor, pipe.audio_encoder, pipe.melspectrogram_shape = old
        del pipe.generation_steps
    assert frames.shape == (9, 64, 64, 3) and not frames.is_cuda and audio.shape == (1, 24000)
    video, fps, aud, afps = read_mjpeg_avi(path, decoder="host")
    assert path.endswith("track.avi") and video.shape == (9, 64, 64, 3) and fps == 6.0 and aud.shape == (1, 24000) and afps == 16000
