"""The band entry points and the caller's buffers, byte for byte: frm_unshuffle_bands against
band_reference.unshuffle on random bytes, through both of its kernels and every condition that
selects one; frm_render_bands and frm_render_bands_batch into a destination 4 bytes into its
allocation, where every byte outside the call's valid rows must keep its sentinel; the alignment
and overlap rules of include/frm.h, each refusal leaving its destination untouched; and the band
count that used to wrap. Frames are at most 1040 x 2 or 40 x 11 texels."""
import ctypes

import numpy as np
import pytest

import band_reference as model
import frm
from frm import _lib
from helpers import params_for

pytestmark = pytest.mark.gpu

SENT = 64        # sentinel bytes on each side of a used span (a multiple of 16: it keeps the alignment)
GUARD = 0xA5     # the sentinels, and everything a render may not write
PAD = 0xC3       # source bytes no reassembly may read
PREFILL = 0x5A   # the destination frame before a reassembly
U32 = 0xFFFFFFFF
OK, BAD, SMALL = _lib.FRM_OK, _lib.FRM_ERR_INVALID_ARGUMENT, _lib.FRM_ERR_BUFFER_TOO_SMALL


def to_device(host):
    import torch

    t = torch.from_numpy(host).to("cuda")
    assert t.data_ptr() % 16 == 0  # offsets below are offsets from a 16-byte boundary
    return t


@pytest.fixture(scope="module")
def renderer(frm_lib):
    """One plain context for every reassembly: frm_unshuffle_bands takes the frame size from it."""
    assert frm.device_count() >= 1
    with frm.Renderer(device=0, max_steps=32) as r:
        r.resize(8, 5)
        r.update_parameters_buffer(params_for(0, 2, frm.POWER8_TIME, 8, 5))
        yield r


class Reassembly:
    """The buffers of one frm_unshuffle_bands case: a source of `ranks` shares, `pad` bytes more
    than rank 0's rows apart, random in its valid rows and PAD everywhere else, between two
    sentinels; a PREFILL destination frame between two sentinels; src_off / dst_off move the
    pointers off their 16-byte boundary."""

    def __init__(self, width, height, band_rows, ranks, pad=0, src_off=0, dst_off=0, seed=1):
        self.geometry = (width, height, band_rows, ranks)
        pitch = width * 4
        self.stride = model.rank_rows(height, band_rows, 0, ranks) * pitch + pad
        self.frame_bytes = height * pitch
        used = ranks * self.stride
        rng = np.random.default_rng(seed)
        self.src_at, self.dst_at = SENT + src_off, SENT + dst_off
        self.host_src = np.full(self.src_at + used + SENT, GUARD, np.uint8)
        span = self.host_src[self.src_at:self.src_at + used]
        span[:] = PAD
        for rank in range(ranks):  # a rank's valid rows come first in its share
            n = model.valid_rows(height, band_rows, rank, ranks) * pitch
            span[rank * self.stride:rank * self.stride + n] = rng.integers(0, 256, n, dtype=np.uint8)
        self.want = model.unshuffle(span, self.stride, width, height, band_rows, ranks)
        host_dst = np.full(self.dst_at + self.frame_bytes + SENT, GUARD, np.uint8)
        host_dst[self.dst_at:self.dst_at + self.frame_bytes] = PREFILL
        self.src, self.dst = to_device(self.host_src), to_device(host_dst)
        self.src_ptr, self.dst_ptr = self.src.data_ptr() + self.src_at, self.dst.data_ptr() + self.dst_at

    def vector_path(self):
        """include/frm.h: 16-byte words iff rows, rank stride and both pointers are 16-byte multiples."""
        return all(v % 16 == 0 for v in (self.geometry[0] * 4, self.stride, self.src_ptr, self.dst_ptr))

    def run_and_check(self, r, stream=None):
        import torch

        width, height, band_rows, ranks = self.geometry
        r.resize(width, height)
        torch.cuda.synchronize()  # the fills above ran on torch's stream
        r.unshuffle_bands(self.src_ptr, self.stride, self.dst_ptr, self.frame_bytes, band_rows, ranks,
                          stream=stream.cuda_stream if stream else 0)
        if stream:
            stream.synchronize()
        r.synchronize()
        got = self.dst.cpu().numpy()
        frame = got[self.dst_at:self.dst_at + self.frame_bytes].reshape(height, width, 4)
        assert np.array_equal(frame, self.want)
        assert (got[:self.dst_at] == GUARD).all() and (got[self.dst_at + self.frame_bytes:] == GUARD).all()
        assert np.array_equal(self.src.cpu().numpy(), self.host_src)


# width, height, band_rows, ranks, the rest of Reassembly's arguments, and the kernel the case must reach
REASSEMBLIES = {
    "vector": (8, 5, 2, 2, {}, True),                        # ragged last band
    "vector_one_word": (4, 3, 1, 3, {}, True),               # rows of a single uint4
    "vector_two_blocks": (1040, 2, 1, 2, {}, True),          # 260 words per row: a second block in x, its bound
    "dword_width_131": (131, 7, 3, 2, {}, False),
    "dword_width_1": (1, 9, 2, 2, {}, False),
    "dword_width_3": (3, 4, 3, 2, {}, False),
    "dword_width_5": (5, 4, 1, 3, {}, False),
    "dword_stride_pad_4": (8, 5, 2, 2, {"pad": 4}, False),   # width divisible by 4, stride no multiple of 16
    "dword_stride_pad_8": (8, 5, 2, 2, {"pad": 8}, False),
    "dword_src_plus_4": (8, 5, 2, 2, {"src_off": 4}, False),  # the stride is a multiple of 16: the pointers decide
    "dword_dst_plus_8": (8, 5, 2, 2, {"dst_off": 8}, False),
    "dword_both_plus_12": (8, 5, 2, 2, {"src_off": 12, "dst_off": 12}, False),
    "one_band": (16, 6, 6, 2, {}, True),                     # rank 1 holds nothing
    "one_band_above_the_height": (16, 6, 9, 2, {}, True),    # a slot of 9 rows for 6
    "more_ranks_than_bands": (8, 4, 2, 5, {}, True),         # three shares never read
    "one_rank": (12, 5, 2, 1, {}, True),                     # a plain copy with a short last band
}


@pytest.mark.parametrize("case", list(REASSEMBLIES))
def test_reassembly_equals_the_reference(renderer, case):
    width, height, band_rows, ranks, more, vector = REASSEMBLIES[case]
    c = Reassembly(width, height, band_rows, ranks, **more)
    assert c.vector_path() == vector  # the case reaches the kernel it is here for
    c.run_and_check(renderer)


def test_reassembly_on_the_callers_stream(renderer):
    import torch

    c = Reassembly(8, 5, 2, 2, seed=2)
    assert c.vector_path()
    c.run_and_check(renderer, stream=torch.cuda.Stream())


# ---- frm_render_bands and frm_render_bands_batch write their rows and nothing else ------------------

W, H, BAND_ROWS, RANKS, STEPS = 40, 11, 4, 2, 32  # bands of 4, 4 and 3 rows: rank 0's second slot has a padding row
PITCH = W * 4
DST_AT = SENT + 4  # the destination: 4 bytes past a 16-byte boundary, inside the contract
GAP = 20           # between a batch's frames


@pytest.fixture(scope="module")
def pose_refs(oracle):
    """(Parameters, oracle frame) of poses P0, P1 and P2: scene 0, 2 iterations."""
    ps = [params_for(0, 2, frm.POWER8_TIME, W, H, pose=pose) for pose in ("P0", "P1", "P2")]
    return [(p, oracle.render(p, W, H, STEPS)) for p in ps]


def guarded_counters():
    """FRM_NUM_COUNTERS words 8 bytes into an int64 tensor, a -1 word on each side."""
    import torch

    return torch.tensor([-1] + [0] * 8 + [-1], dtype=torch.int64, device="cuda")


def check_counters(t, refs):
    got = [int(v) for v in t.cpu().tolist()]
    assert got[0] == -1 and got[9] == -1
    assert got[1:8] == [sum(int(ref["counters"][i]) for ref in refs) for i in range(7)]


def check_rank_rows(body, rank, rgba):
    """body: the rank's local rows. Frame rows where global_row places them, padding untouched."""
    rows = model.rank_rows(H, BAND_ROWS, rank, RANKS)
    body = body.reshape(rows, W, 4)
    padding = 0
    for local in range(rows):
        y = model.global_row(local, H, BAND_ROWS, rank, RANKS)
        if y < 0:
            padding += 1
            assert (body[local] == GUARD).all(), f"rank {rank}: padding row {local} written"
        else:
            assert np.array_equal(body[local], rgba[y]), f"rank {rank}: local row {local}, frame row {y}"
    assert padding == rows - model.valid_rows(H, BAND_ROWS, rank, RANKS)


@pytest.mark.parametrize("kernel", ["persistent", "simple"])
def test_render_bands_writes_its_valid_rows_and_nothing_else(frm_lib, pose_refs, kernel):
    import torch

    assert model.valid_rows(H, BAND_ROWS, 0, RANKS) == 7 and model.rank_rows(H, BAND_ROWS, 0, RANKS) == 8
    p, ref = pose_refs[1]
    assert ref["counters"][1] > 0  # the frame shows the scene: hit pixels
    flags = frm.FRM_FLAG_PERSISTENT_KERNEL if kernel == "persistent" else frm.FRM_FLAG_SIMPLE_KERNEL
    rds = [frm.Renderer(device=0, max_steps=STEPS, flags=flags) for _ in range(RANKS)]  # a context per rank: its
    try:                                                                               # second launch has history
        for rd in rds:
            rd.resize(W, H)
            rd.update_parameters_buffer(p)
        for launch in range(2 if kernel == "persistent" else 1):  # the second one fetches in the scheduled order
            counters = guarded_counters()
            need = [model.rank_rows(H, BAND_ROWS, rank, RANKS) * PITCH for rank in range(RANKS)]
            bufs = [torch.full((DST_AT + n + SENT,), GUARD, dtype=torch.uint8, device="cuda") for n in need]
            assert all(b.data_ptr() % 16 == 0 for b in bufs)
            torch.cuda.synchronize()
            for rank, rd in enumerate(rds):
                rd.render_bands(bufs[rank].data_ptr() + DST_AT, need[rank], BAND_ROWS, rank, RANKS, 0,
                                counters.data_ptr() + 8)
            for rd in rds:
                rd.synchronize()
            for rank in range(RANKS):
                got = bufs[rank].cpu().numpy()
                check_rank_rows(got[DST_AT:DST_AT + need[rank]], rank, ref["rgba"])
                assert (got[:DST_AT] == GUARD).all() and (got[DST_AT + need[rank]:] == GUARD).all()
            check_counters(counters, [ref])
    finally:
        for rd in rds:
            rd.close()


@pytest.mark.parametrize("kernel", ["persistent", "simple"])
def test_render_bands_batch_writes_its_valid_rows_and_nothing_else(frm_lib, pose_refs, kernel):
    import torch

    ps, refs = [p for p, _ in pose_refs], [ref for _, ref in pose_refs]
    flags = frm.FRM_FLAG_PERSISTENT_KERNEL if kernel == "persistent" else frm.FRM_FLAG_SIMPLE_KERNEL
    rds = [frm.Renderer(device=0, max_steps=STEPS, flags=flags) for _ in range(RANKS)]
    try:
        for rd in rds:
            rd.resize(W, H)
        for launch in range(2 if kernel == "persistent" else 1):
            counters = guarded_counters()
            need = [model.rank_rows(H, BAND_ROWS, rank, RANKS) * PITCH for rank in range(RANKS)]
            span = [(len(ps) - 1) * (n + GAP) + n for n in need]  # the last frame has no gap behind it
            bufs = [torch.full((DST_AT + s + SENT,), GUARD, dtype=torch.uint8, device="cuda") for s in span]
            assert all(b.data_ptr() % 16 == 0 for b in bufs)
            torch.cuda.synchronize()
            for rank, rd in enumerate(rds):
                rd.render_bands_batch(ps, bufs[rank].data_ptr() + DST_AT, dst_bytes=span[rank],
                                      frame_stride=need[rank] + GAP, band_rows=BAND_ROWS, first_band=rank,
                                      band_stride=RANKS, dev_counters=counters.data_ptr() + 8)
            for rd in rds:
                rd.synchronize()
            for rank in range(RANKS):
                got = bufs[rank].cpu().numpy()
                assert (got[:DST_AT] == GUARD).all() and (got[DST_AT + span[rank]:] == GUARD).all()
                for k, ref in enumerate(refs):
                    at = DST_AT + k * (need[rank] + GAP)
                    check_rank_rows(got[at:at + need[rank]], rank, ref["rgba"])
                    if k + 1 < len(refs):
                        assert (got[at + need[rank]:at + need[rank] + GAP] == GUARD).all(), f"gap after frame {k}"
            check_counters(counters, refs)
    finally:
        for rd in rds:
            rd.close()


# ---- the contract's refusals: a status, and nothing launched ------------------------------------------

def test_refusals_launch_nothing(frm_lib):
    """8 x 5 texels in bands of 2 over 2 ranks, shares 128 bytes apart: the reassembly reads
    [0, 192) of its source. Every refused call leaves the whole GUARD allocation as it was."""
    import torch

    width, height, band_rows, ranks, stride, frame = 8, 5, 2, 2, 128, 160
    assert model.rank_rows(height, band_rows, 0, ranks) * width * 4 == stride
    extent = model.read_extent(stride, width, height, band_rows, ranks)
    assert extent == 192
    p = params_for(0, 2, frm.POWER8_TIME, width, height)
    params = (_lib.FrmParameters * 2)()
    for k in range(2):
        ctypes.memmove(ctypes.addressof(params[k]), p.to_bytes(), ctypes.sizeof(_lib.FrmParameters))
    arena = torch.full((1024,), GUARD, dtype=torch.uint8, device="cuda")  # source and destinations of every call
    words = torch.zeros(10, dtype=torch.int64, device="cuda")
    a, cnt = arena.data_ptr(), words.data_ptr()
    assert a % 16 == 0 and cnt % 8 == 0
    with frm.Renderer(device=0, max_steps=STEPS) as r:
        L, ctx = r._lib, r.ctx
        r.resize(width, height)
        r.update_parameters_buffer(p)
        torch.cuda.synchronize()

        def untouched():
            r.synchronize()
            return bool((arena == GUARD).all()) and int(words.abs().sum()) == 0

        def bands(dst, dst_bytes=stride, counters=None):
            return L.frm_render_bands(ctx, dst, dst_bytes, band_rows, 0, ranks, None, counters), untouched()

        def batch(dst, dst_bytes=2 * stride, counters=None):
            return (L.frm_render_bands_batch(ctx, 2, ctypes.addressof(params), dst, dst_bytes, stride, band_rows, 0,
                                             ranks, None, counters), untouched())

        def unshuffle(src, dst, dst_bytes=frame):
            return L.frm_unshuffle_bands(ctx, src, stride, dst, dst_bytes, band_rows, ranks, None), untouched()

        assert bands(a + 1) == (BAD, True)
        assert bands(a + 2) == (BAD, True)
        assert bands(a, counters=cnt + 4) == (BAD, True)
        assert batch(a + 1) == (BAD, True)
        assert batch(a + 2) == (BAD, True)
        assert batch(a, counters=cnt + 4) == (BAD, True)
        assert unshuffle(a + 2, a + 512) == (BAD, True)
        assert unshuffle(a, a + 512 + 1) == (BAD, True)
        assert unshuffle(a, a + 512 + 2) == (BAD, True)
        assert unshuffle(a, a + extent - 4) == (BAD, True)      # the frame starts on the last texel read
        assert unshuffle(a + 512, a + 512 - 4) == (BAD, True)   # the frame ends on the first texel read
        # two faults at once: the size, checked first today, is still reported first
        assert bands(a + 1, dst_bytes=stride - 4) == (SMALL, True)
        assert batch(a + 1, dst_bytes=2 * stride - 4) == (SMALL, True)
        assert unshuffle(a, a + 512 + 1, dst_bytes=frame - 4) == (SMALL, True)

    # one byte past the last byte read: accepted, and the frame is right
    c = Reassembly(width, height, band_rows, ranks, seed=3)
    both = np.full(SENT + extent + frame + SENT, GUARD, np.uint8)
    both[SENT:SENT + extent] = c.host_src[c.src_at:c.src_at + extent]
    both[SENT + extent:SENT + extent + frame] = PREFILL
    dev = to_device(both)
    with frm.Renderer(device=0, max_steps=STEPS) as r:
        r.resize(width, height)
        torch.cuda.synchronize()
        src = dev.data_ptr() + SENT
        assert r._lib.frm_unshuffle_bands(r.ctx, src, stride, src + extent, frame, band_rows, ranks, None) == OK
        r.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(got[SENT + extent:SENT + extent + frame].reshape(height, width, 4), c.want)
    assert np.array_equal(got[:SENT + extent], both[:SENT + extent]) and (got[SENT + extent + frame:] == GUARD).all()


def test_a_band_count_that_used_to_wrap(frm_lib):
    """band_rows = 0xFFFFFFFF on an 8 x 2 frame: one band in a slot of 0xFFFFFFFF rows. With
    (height + band_rows - 1) / band_rows it counted as no band: the render succeeded without
    rendering and the reassembly skipped its stride check."""
    import torch

    width, height = 8, 2
    p = params_for(0, 2, frm.POWER8_TIME, width, height)
    dst = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda")
    src = torch.full((128,), GUARD, dtype=torch.uint8, device="cuda")
    with frm.Renderer(device=0, max_steps=STEPS) as r:
        r.resize(width, height)
        r.update_parameters_buffer(p)
        torch.cuda.synchronize()
        assert r._lib.frm_render_bands(r.ctx, dst.data_ptr(), 64, U32, 0, 1, None, None) == SMALL
        r.synchronize()
        assert bool((dst == GUARD).all())
        assert r._lib.frm_unshuffle_bands(r.ctx, src.data_ptr(), 64, dst.data_ptr(), 64, U32, 2, None) == BAD
        assert b"rank stride" in r._lib.frm_last_error(r.ctx)
        r.synchronize()
        assert bool((dst == GUARD).all())
