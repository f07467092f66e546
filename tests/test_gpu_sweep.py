"""The appearance sweep on the device (include/crnerf_sweep.h): one content grid decoded under S styles, against S single decodes BIT FOR BIT.

Inputs are tests/_crossray_cases.decode_case's (the decoder "that sees", contrast 4000).  The content grid is decode_case(HW, 1024)["content"] and
the weights are decode_case's at its default seed, shared by every style.  decode_case draws its grids from a generator seeded by (HW, HWs) alone
-- its `seed` argument reaches only the weights -- so "style s" cannot be decode_case(HW, 1024, seed=11 + s)["style"]: those S arrays are one
and the same array, and a test of S equal styles cannot tell image s from image t.  Style s is decode_case(1 + s, HWs)["style"] instead: the
same function, S different generator seeds, S different grids (asserted below).

1. ops.crossray_decode_multi(x, stats, w)[s] == ops.crossray_decode(x, style_s, w) (torch.equal) at HW in {1, 63, 64, 65, 4096, 4097, 131073}
   -- the 4-lane tail of the apply pass, both sides of the Gram reduction's switch, one pixel past the 2,048-workgroup grid stride -- for
   S in {1, 2, 3, 16}; the style grid on the large path (HWs = 4097) at HW = 4097; 17 styles through the Python split.
2. A style's image does not depend on its neighbours: a permuted style list permutes the images, a style listed twice gives two equal images.
3. Stats made for content_hw = 4096 refuse a grid of 4,097 pixels.
4. u8=True equals (float.clamp(0, 1) * 255).to(uint8) rearranged to [S,HW,3], byte for byte, into a view whose frames are padded (the pad
   bytes stay as they were); a NaN content grid stores 0 in every byte.
5. Each image of S = 3 at (4097, 1024) is within decode_reference's bar of the float64 oracle (the bar of tests/test_gpu_crossray_exact.py).
6. video.render_appearance_sweep(...)[s][i] == video.render_video(..., style_img=photo_s)[i] byte for byte on synthetic models, on both sides
   of the switch, for precision=None and lean=True; kept features decode to the same bytes; rank 1 of 2 returns the odd frames.
7. The sweep renders each frame once: pipeline.batched_inference is called 3 times for 3 frames and 3 styles, not 9."""
import numpy as np
import pytest
import torch

import _crossray_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HWS = (1, 63, 64, 65, 4096, 4097, 131073)
SS = (1, 2, 3, 16)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_weights, _styles, _content, _single = {}, {}, {}, {}


def weights():
    if "w" not in _weights:
        _weights["w"] = [T(t) for t in C.decode_case(1, 1)["weights"]]
    return _weights["w"]


def style(s, HWs=1024):
    if (s, HWs) not in _styles:
        _styles[(s, HWs)] = T(C.decode_case(1 + s, HWs)["style"])
    return _styles[(s, HWs)]


def content(HW):
    if HW not in _content:
        _content[HW] = T(C.decode_case(HW, 1024)["content"])
    return _content[HW]


def single(HW, s, HWs=1024):
    """ops.crossray_decode(content, style_s): the reference of the bit-for-bit tests, computed once per (HW, s, HWs)."""
    from crnerf_amd import ops
    key = (HW, s, HWs)
    if key not in _single:
        with torch.no_grad():
            _single[key] = ops.crossray_decode(content(HW), style(s, HWs), weights()).clone()
    return _single[key]


def test_the_styles_differ():
    assert len({style(s).cpu().numpy().tobytes() for s in range(17)}) == 17
    a, b = C.decode_case(65, 1024, seed=11)["style"], C.decode_case(65, 1024, seed=12)["style"]
    assert np.array_equal(a, b)          # why style s is not decode_case(HW, 1024, seed=11 + s)["style"] (module docstring)


# ------------------------------------------------------------------------------------------------------------------ 1. bit identity, float
@torch.no_grad()
@pytest.mark.parametrize("HW", HWS)
def test_multi_decode_equals_single_decodes(HW):
    from crnerf_amd import ops
    x, w = content(HW), weights()
    for S in SS:
        stats = ops.crossray_style_stats([style(s) for s in range(S)], w, HW)
        assert (stats.S, stats.style_hw, stats.small_path) == (S, 1024, HW <= 4096) and tuple(stats.stats.shape) == (S, 1088)
        got = ops.crossray_decode_multi(x, stats, w)
        assert tuple(got.shape) == (S, 3, HW) and got.dtype == torch.float32
        for s in range(S):
            assert torch.equal(got[s], single(HW, s)), "HW %d, S %d: image %d differs from the single decode" % (HW, S, s)


@torch.no_grad()
def test_stats_are_what_the_single_decode_leaves_in_its_workspace():
    from crnerf_amd import ops
    w = weights()
    for HW in (65, 4097):
        stats = ops.crossray_style_stats([style(s) for s in range(3)], w, HW)
        for s in range(3):
            ops.crossray_decode(content(HW), style(s), w)
            st = ops.crossray_workspace(torch.device(DEV)).view(torch.float32)[C.WS_STATS:]
            assert torch.equal(stats.stats[s, :64], st[64:128])                          # ST_SMEAN
            assert torch.equal(stats.stats[s, 64:], st[128 + 3072:128 + 4096])           # ST_SMAT


@torch.no_grad()
@pytest.mark.parametrize("HW", (1000, 4097))
def test_style_grid_on_the_large_path(HW):
    """HWs = 4097: the style job runs one tile per wave, and a content grid of <= 4096 pixels follows it onto the two-launch reduction."""
    from crnerf_amd import ops
    x, w = content(HW), weights()
    stats = ops.crossray_style_stats([style(s, 4097) for s in range(3)], w, HW)
    assert not stats.small_path and stats.style_hw == 4097
    got = ops.crossray_decode_multi(x, stats, w)
    for s in range(3):
        assert torch.equal(got[s], single(HW, s, 4097))


@torch.no_grad()
def test_seventeen_styles_through_the_python_split():
    from crnerf_amd import ops
    HW, x, w = 65, content(65), weights()
    stats = ops.crossray_style_stats(torch.stack([style(s) for s in range(17)]), w, HW)
    got = ops.crossray_decode_multi(x, stats, w)
    assert tuple(got.shape) == (17, 3, HW)
    for s in range(17):
        assert torch.equal(got[s], single(HW, s))
    u8 = ops.crossray_decode_multi(x, stats, w, u8=True)
    assert torch.equal(u8, (got.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------------ 2. no neighbours
@torch.no_grad()
@pytest.mark.parametrize("HW", (65, 4097))
def test_an_image_does_not_depend_on_the_other_styles(HW):
    from crnerf_amd import ops
    x, w = content(HW), weights()
    order = [2, 0, 3, 1, 2]                                 # a permutation of 0..3, and style 2 twice
    got = ops.crossray_decode_multi(x, ops.crossray_style_stats([style(s) for s in order], w, HW), w)
    base = ops.crossray_decode_multi(x, ops.crossray_style_stats([style(s) for s in range(4)], w, HW), w)
    for i, s in enumerate(order):
        assert torch.equal(got[i], base[s])
    assert torch.equal(got[0], got[4])
    assert not torch.equal(base[0], base[1])


# ------------------------------------------------------------------------------------------------------------------ 3. the other path
@torch.no_grad()
def test_stats_of_the_other_reduction_path_are_refused():
    from crnerf_amd import ops
    w = weights()
    stats = ops.crossray_style_stats([style(0), style(1)], w, 4096)
    with pytest.raises(ValueError, match="another order"):
        ops.crossray_decode_multi(content(4097), stats, w)
    ops.crossray_decode_multi(content(65), stats, w)       # any size on the same side is fine


# ------------------------------------------------------------------------------------------------------------------ 4. uint8
@torch.no_grad()
@pytest.mark.parametrize("HW", (1, 65, 4097))
def test_uint8_frames_into_a_padded_view(HW):
    from crnerf_amd import ops
    x, w, S = content(HW), weights(), 3
    stats = ops.crossray_style_stats([style(s) for s in range(S)], w, HW)
    f = ops.crossray_decode_multi(x, stats, w)
    want = (f.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 1).contiguous()           # [S,HW,3]
    buf = torch.full((S, HW + 5, 3), 77, dtype=torch.uint8, device=DEV)
    out = ops.crossray_decode_multi(x, stats, w, out=buf[:, :HW], u8=True)
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == 3 * (HW + 5)
    assert torch.equal(buf[:, :HW], want) and bool((buf[:, HW:] == 77).all())
    assert torch.equal(ops.crossray_decode_multi(x, stats, w, u8=True), want)
    assert len(torch.unique(want)) > (1 if HW == 1 else 8)                               # images, not constants
    # the float planes into a view padded between planes and between images
    fbuf = torch.full((S, 3, HW + 3), float("nan"), device=DEV)
    ops.crossray_decode_multi(x, stats, w, out=fbuf[:, :, :HW])
    assert torch.equal(fbuf[:, :, :HW], f) and bool(torch.isnan(fbuf[:, :, HW:]).all())


@torch.no_grad()
def test_uint8_stores_zero_for_nan():
    from crnerf_amd import ops
    HW, w = 65, weights()
    x = torch.full((HW, 64), float("nan"), device=DEV)
    stats = ops.crossray_style_stats([style(0), style(1)], w, HW)
    assert bool(torch.isnan(ops.crossray_decode_multi(x, stats, w)).all())               # every decoded pixel is NaN
    out = ops.crossray_decode_multi(x, stats, w, out=torch.full((2, HW, 3), 77, dtype=torch.uint8, device=DEV), u8=True)
    assert bool((out == 0).all())


@torch.no_grad()
def test_out_of_the_wrong_shape_or_layout_is_refused():
    from crnerf_amd import ops
    HW, w = 65, weights()
    x, stats = content(HW), ops.crossray_style_stats([style(0), style(1)], w, HW)
    for bad, u8 in ((torch.empty(2, 3, HW + 1, device=DEV), False), (torch.empty(2, HW, 3, device=DEV), True),
                    (torch.empty(2, HW, 3, device=DEV).permute(0, 2, 1), False), (torch.empty(2, 3, HW, dtype=torch.uint8, device=DEV).permute(0, 2, 1), True)):
        with pytest.raises(ValueError, match="out"):
            ops.crossray_decode_multi(x, stats, w, out=bad, u8=u8)


# ------------------------------------------------------------------------------------------------------------------ 5. against float64
@torch.no_grad()
def test_each_image_against_float64():
    from crnerf_amd import ops
    HW, HWs, S, w = 4097, 1024, 3, weights()
    case = C.decode_case(HW, HWs)
    got = ops.crossray_decode_multi(content(HW), ops.crossray_style_stats([style(s) for s in range(S)], w, HW), w).cpu().double()
    for s in range(S):
        ref, own, bar = C.decode_reference(dict(case, style=style(s).cpu().numpy()))
        err = float((got[s] - torch.from_numpy(ref)).abs().max())
        print("\nstyle %d at (%d, %d): max |rgb - float64| %.2e, bar %.1e (fp32 CPU oracle %.2e)" % (s, HW, HWs, err, bar, own))
        assert err <= bar


# ------------------------------------------------------------------------------------------------------------------ 6., 7. the sweep
class _HP:
    nerf_out_dim, pertubeCord = 64, False
    N_emb_xyz, N_emb_dir, N_samples, N_importance, use_disp, encode_a, encode_random, N_a = 15, 4, 8, 8, False, True, True, 48

    def __init__(self, img_wh):
        self.img_wh = list(img_wh)


_scene = {}


def scene(img_wh):
    """Synthetic models (the states of test_orchestration_mirror_video_frame_and_checkpoint_prefixes; the decoder at the contrast "that sees" --
    at the default contrast every frame of every style is one flat colour, and equal bytes show nothing), three style photos, and the three
    videos render_video makes of them: the reference of the sweep tests, rendered once per image size and precision."""
    import crnerf_amd.synth as synth
    from crnerf_amd import pipeline
    if img_wh not in _scene:
        hp = _HP(img_wh)
        models, emb = pipeline.get_model(hp, DEV), pipeline.get_embeddings(hp)
        enc_a = pipeline.encoder_sameoutputsize(64).to(DEV)
        for m, st in ((models["coarse"], synth.mlp_state(61, 3.0, 1.0)), (models["fine"], synth.mlp_state(62, 3.0, 1.0)),
                      (models["decoder"], synth.decoder_state(63, contrast=C.SEEING)), (enc_a, synth.encoder_state(64, 2.0))):
            state = m.state_dict()
            state.update({k: torch.from_numpy(v) for k, v in st.items()})
            m.load_state_dict(state)
        rng = np.random.default_rng(3)
        photos = [T(rng.uniform(0, 1, (1, 3, 40, 56)).astype(np.float32)) for _ in range(3)]
        _scene[img_wh] = dict(hp=hp, models=models, emb=emb, enc_a=enc_a, photos=photos, videos={})
    return _scene[img_wh]


def videos(sc, lean):
    from crnerf_amd import video
    if lean not in sc["videos"]:
        sc["videos"][lean] = [video.render_video(sc["models"], sc["emb"], sc["enc_a"], p, sc["hp"], n_frames=3, chunk=1000, lean=lean) for p in sc["photos"]]
    return sc["videos"][lean]


@torch.no_grad()
@pytest.mark.parametrize("lean", (False, True))
@pytest.mark.parametrize("img_wh", ((16, 12), (72, 60)))
def test_the_sweep_equals_S_videos(img_wh, lean):
    from crnerf_amd import pipeline, video
    sc = scene(img_wh)
    want = videos(sc, lean)
    got, feats = video.render_appearance_sweep(sc["models"], sc["emb"], sc["enc_a"], sc["photos"], sc["hp"], n_frames=3, chunk=1000, lean=lean,
                                               keep_features=True)
    w, h = img_wh
    assert sorted(got) == [0, 1, 2] and sorted(feats) == [0, 1, 2]
    for s in range(3):
        assert sorted(got[s]) == [0, 1, 2]
        for i in range(3):
            assert got[s][i].dtype == np.uint8 and got[s][i].shape == (h, w, 3)
            assert np.array_equal(got[s][i], want[s][i]), "style %d frame %d" % (s, i)
    assert not np.array_equal(got[0][0], got[1][0]) and not np.array_equal(got[0][0], got[0][1])
    # a kept feature grid decodes to the same bytes without a render -- under a style list in another order, as for a photo that arrives later
    stats = sc["models"]["decoder"].style_stats([sc["enc_a"](sc["photos"][s]) for s in (2, 0)], (h, w))
    for i in range(3):
        assert tuple(feats[i].shape) == (h * w, 64)
        again = pipeline.decode_frame_styles(sc["models"], feats[i], h, w, stats).cpu().numpy()
        assert np.array_equal(again[0], want[2][i]) and np.array_equal(again[1], want[0][i])


def test_rank_one_of_two_renders_the_odd_frames_and_each_frame_once(monkeypatch):
    from crnerf_amd import pipeline, video
    sc = scene((16, 12))
    want = videos(sc, False)
    calls = []
    inner = pipeline.batched_inference
    monkeypatch.setattr(pipeline, "batched_inference", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    got = video.render_appearance_sweep(sc["models"], sc["emb"], sc["enc_a"], sc["photos"], sc["hp"], n_frames=3, chunk=1000)
    assert len(calls) == 3                                   # 3 frames x 3 styles: 3 renders, not 9
    assert all(np.array_equal(got[s][i], want[s][i]) for s in range(3) for i in range(3))
    del calls[:]
    odd = video.render_appearance_sweep(sc["models"], sc["emb"], sc["enc_a"], sc["photos"], sc["hp"], n_frames=4, rank=1, world_size=2, chunk=1000)
    assert len(calls) == 2 and all(sorted(odd[s]) == [1, 3] for s in range(3))
    full = video.render_video(sc["models"], sc["emb"], sc["enc_a"], sc["photos"][1], sc["hp"], n_frames=4, rank=1, world_size=2, chunk=1000)
    assert sorted(full) == [1, 3] and all(np.array_equal(odd[1][i], full[i]) for i in (1, 3))


def test_grad_mode_with_trainable_weights_is_refused():
    from crnerf_amd import ops
    w = [t.clone().requires_grad_(True) for t in weights()]
    with pytest.raises(ValueError, match="inference"):
        ops.crossray_style_stats([style(0)], w, 65)
    with torch.no_grad():
        stats = ops.crossray_style_stats([style(0)], w, 65)
    with pytest.raises(ValueError, match="inference"):
        ops.crossray_decode_multi(content(65), stats, w)
