"""CPU: audio.chunk_plan, the planner of long-form conversion (DESIGN.md "Long-form conversion").

All lengths are mel frames of hop = 256 samples at 24 kHz; Cb, Lc, Rc are multiples of 15 frames. A cut exists at
k * Cb for k >= 1 while k * Cb + Rc < T_song."""
import pytest

from svc_inference_pipeline_amd import audio as A
from svc_inference_pipeline_amd.runtime import mel_frames

HOP, FS, FADE = 256, 24000, 20 * 256


def range_rule(st):
    """svc_stitch's range rule on a StitchPlan, written out again from the issue's definitions."""
    B = len(st.n)
    for b in range(B):
        d_lo, d_hi = (-st.search, max(st.search - 1, 0)) if st.joined[b] else (0, 0)
        reads = [st.lead[b] + d_lo, st.lead[b] + d_hi + st.body[b] - 1]            # as the chunk that plays
        if st.joined[b]:
            reads += [st.lead[b] - st.search, st.lead[b] + d_hi + st.xfade - 1]      # its candidates' windows
        if b + 1 < B and st.joined[b + 1]:
            reads += [st.lead[b] + d_lo + st.body[b], st.lead[b] + d_hi + st.body[b] + st.xfade - 1]  # as predecessor
        assert min(reads) >= 0 and max(reads) < st.n[b], (b, reads, st.n[b])


def check_plan(p, N, n16):
    T = mel_frames(N, 1024, HOP)
    assert p.T_song == T and p.chunks == len(p.start) == len(p.frames) == len(p.body) == len(p.rows24) == len(p.rows16)
    assert p.Cb % 15 == 0 and p.Lc % 15 == 0 and p.Rc % 15 == 0 and p.Cb >= 15
    # the bodies tile [0, T_song)
    assert p.body[0][0] == 0 and p.body[-1][1] == T
    for k in range(p.chunks - 1):
        assert p.body[k][1] == p.body[k + 1][0] == (k + 1) * p.Cb
    for k in range(p.chunks):
        last = k == p.chunks - 1
        s = p.start[k]
        assert s == max(0, k * p.Cb - p.Lc) and s % 15 == 0 and (p.body[k][0] - s) % 15 == 0
        end = T if last else (k + 1) * p.Cb + p.Rc
        assert p.frames[k] == end - s
        lo, hi = p.rows24[k]
        assert lo == s * HOP and hi == (N if last else end * HOP)
        assert mel_frames(hi - lo, 1024, HOP) == p.frames[k]  # the chunk's own frame count, as convert_ragged sees it
        lo16, hi16 = p.rows16[k]
        assert lo16 * 3 == lo * 2 or lo16 == n16  # whole samples: the same interval times 2 / 3 (or clipped)
        assert hi16 == (n16 if last else min(hi * 2 // 3, n16)) and (last or (hi * 2) % 3 == 0)
        assert 0 <= lo16 <= hi16 <= n16
        st = p.stitch
        assert st.n[k] == p.frames[k] * HOP - (0 if last else FADE)
        assert st.lead[k] == (p.body[k][0] - s) * HOP and st.out_off[k] == p.body[k][0] * HOP
        assert st.joined[k] == (1 if k else 0)
        tail = max(st.search - 1, 0) if last and k else 0  # a joined last chunk cannot be displaced past its row's end
        assert st.body[k] == (p.body[k][1] - p.body[k][0]) * HOP - tail
    assert p.stitch.out_len == T * HOP
    range_rule(p.stitch)
    A.check_stitch_plan(p.stitch)


@pytest.mark.parametrize("clip_s,context_s", [(10.0, 0.64), (0.8, 0.32), (0.16, 0.3), (1.0, 1.3)])
def test_plans_around_every_boundary(clip_s, context_s):
    """Song lengths around every cut's appearance (k Cb + Rc and one frame more), around whole frames, and T_song < 15."""
    p0 = A.chunk_plan(FS, FS, HOP, 1024, clip_s, context_s)
    Cb, Rc = p0.Cb, p0.Rc
    # 0.8 s is 75 frames exactly (not 74.99..), 0.3 s is 28.125 frames and rounds up to 30, 1 s is 93.75 and rounds down
    assert (Cb, Rc) == {(10.0, 0.64): (930, 60), (0.8, 0.32): (75, 30), (0.16, 0.3): (15, 30), (1.0, 1.3): (90, 135)}[
        (clip_s, context_s)]
    frames = {1, 7, 14, 15, 16, Cb, Cb + 1}
    for k in (1, 2, 3, 5):
        frames |= {k * Cb + Rc - 1, k * Cb + Rc, k * Cb + Rc + 1, k * Cb + Rc + 2, (k + 1) * Cb, (k + 1) * Cb - 1}
    for T in sorted(frames):
        for extra in (0, 1, 255):
            N = T * HOP + extra
            n16 = N * 2 // 3
            p = A.chunk_plan(N, FS, HOP, 1024, clip_s, context_s, n16=n16)
            check_plan(p, N, n16)
            want = 1 + sum(1 for k in range(1, 10000) if k * Cb + Rc < T)
            assert p.chunks == want, (T, p.chunks, want)


def test_one_and_two_chunks():
    p = A.chunk_plan(FS, FS, HOP, 1024, 0.8, 0.32)
    Cb, Rc = p.Cb, p.Rc
    assert (Cb, p.Lc, Rc) == (75, 30, 30)
    assert A.chunk_plan((Cb + Rc) * HOP, FS, HOP, 1024, 0.8, 0.32).chunks == 1
    two = A.chunk_plan((Cb + Rc + 1) * HOP, FS, HOP, 1024, 0.8, 0.32)
    assert two.chunks == 2 and two.frames == [Cb + Rc, Rc + 1 + p.Lc] and two.body == [(0, 75), (75, 106)]
    tiny = A.chunk_plan(14 * HOP + 3, FS, HOP, 1024, 0.8, 0.32)  # T_song < 15: one chunk, the song itself
    assert tiny.chunks == 1 and tiny.frames == [14] and tiny.rows24 == [(0, 14 * HOP + 3)]
    assert tiny.stitch.n == [14 * HOP] and tiny.stitch.body == [14 * HOP] and tiny.stitch.joined == [0]


def test_defaults_and_the_issue_example():
    d = A.chunk_plan(180 * FS)
    assert (d.Cb, d.Lc, d.Rc, d.stitch.xfade, d.stitch.search) == (930, 60, 60, 1024, 192)
    p = A.chunk_plan(3 * FS, clip_s=0.8, context_s=0.32)  # the GPU test's song
    assert p.chunks == 4 and p.body == [(0, 75), (75, 150), (150, 225), (225, 281)]
    # float 16 kHz rows of their own length, and a 16 kHz signal a little shorter than 2 / 3 of the song
    q = A.chunk_plan(3 * FS, clip_s=0.8, context_s=0.32, n16=47990, n16_float=48000)
    assert q.rows16[-1] == (33280, 47990) and q.rows16_float[-1] == (33280, 48000) and q.rows16[0] == q.rows16_float[0]
    assert A.chunk_plan(3 * FS, clip_s=0.8, context_s=0.32).rows16_float is None


def test_value_errors():
    ok = dict(fs=FS, hop=HOP, n_fft=1024, clip_s=0.8, context_s=0.32)
    A.chunk_plan(3 * FS, **ok)
    # Rc * hop >= X + R + 20 hop: 30 frames = 7680 samples hold 1024 + 192 + 5120 = 6336, not 2400 + ...
    with pytest.raises(ValueError, match="right context"):
        A.chunk_plan(3 * FS, **{**ok, "context_s": 0.16})          # 15 frames = 3840 samples
    with pytest.raises(ValueError, match="right context"):
        A.chunk_plan(3 * FS, xfade=2400, **ok)                      # 2400 + 192 + 5120 > 7680
    # (Lc * hop >= R cannot fail on its own: Lc = Rc, and the rule above already asks more of Rc)
    with pytest.raises(ValueError, match="right context"):
        A.chunk_plan(3 * FS, **{**ok, "context_s": 0.0}, search=1, xfade=1)
    with pytest.raises(ValueError, match="shortest body"):
        A.chunk_plan(3 * FS, xfade=15 * HOP + 1, search=0, **{**ok, "context_s": 0.64})
    A.chunk_plan(3 * FS, xfade=15 * HOP, search=0, **{**ok, "context_s": 0.64})
    for kw in (dict(xfade=0), dict(xfade=8193), dict(search=-1), dict(search=1025)):
        with pytest.raises(ValueError, match="xfade"):
            A.chunk_plan(3 * FS, **ok, **kw)
    with pytest.raises(ValueError, match="more than 4096 chunks"):
        A.chunk_plan((4096 * 15 + 30 + 1) * HOP, FS, HOP, 1024, 0.16, 0.32)
    assert A.chunk_plan((4096 * 15 + 30) * HOP, FS, HOP, 1024, 0.16, 0.32).chunks == 4096
    for u in (-1, 1 << 19):
        with pytest.raises(ValueError, match="utterance id"):
            A.chunk_plan(3 * FS, utt_id=u, **ok)
    with pytest.raises(ValueError, match="less than one frame"):
        A.chunk_plan(HOP - 1, **ok)
    with pytest.raises(ValueError, match="clip_s"):
        A.chunk_plan(3 * FS, **{**ok, "clip_s": 0.0})


def test_noise_ids():
    p = A.chunk_plan(3 * FS, clip_s=0.8, context_s=0.32, utt_id=5)
    assert p.noise_ids == [(5 << 12) | k for k in range(4)]
    top = A.chunk_plan(3 * FS, clip_s=0.8, context_s=0.32, utt_id=(1 << 19) - 1)
    assert max(top.noise_ids) < 2 ** 31 and top.noise_ids[0] == ((1 << 19) - 1) << 12  # an int32 utterance id


def test_merge_stitch_plans():
    a = A.chunk_plan(3 * FS, clip_s=0.8, context_s=0.32).stitch
    b = A.chunk_plan(FS * 3 // 2, clip_s=0.8, context_s=0.32).stitch  # 140 frames: two chunks
    m = A.merge_stitch_plans([a, b], a.out_len)
    assert m.out_len == 2 * a.out_len and m.joined == [0, 1, 1, 1, 0, 1]
    assert m.out_off == a.out_off + [a.out_len + v for v in b.out_off] and m.n == a.n + b.n
    A.check_stitch_plan(m)
    range_rule(m)
    with pytest.raises(ValueError):
        A.merge_stitch_plans([a, b], b.out_len)
    with pytest.raises(ValueError):
        A.merge_stitch_plans([a, b._replace(search=8)], a.out_len)
