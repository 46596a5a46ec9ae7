"""Device hop payload round trip (hop.hip) in one process: the sender's kernel stores into
this GPU's own inbox, the receiver's kernel unpacks it.  Pins the payload encodings the
multi-rank pipeline uses: f32 words bit-exact, bf16 pairs equal to round-to-nearest-even
of the f32 hidden, header words raw, sequence tags advancing across messages.  The bulk
hop the split UNet uses: segments at their offsets bit for bit, the unrolled copy and its
tail, the arrival counter and sequence words, graph replay, and what both refuse.  Every
receive follows its send on one stream with a bound of 5 s, so a broken send fails a test
through the error word."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Self:
    """A 'peer inbox' that is this process's own inbox (no IPC mapping needed)."""

    def __init__(self, inbox):
        self.ptr = inbox.ptr


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("H", [64, 4096, 8192])
def test_hop_roundtrip_payload(cuda, bf16, H):
    from cake_amd.parallel import hop
    nhdr = 16
    inbox = hop.Inbox(hop.hop_words(H, nhdr, bf16))
    try:
        sseq = torch.zeros(1, dtype=torch.int32, device=cuda)
        rseq = torch.zeros(1, dtype=torch.int32, device=cuda)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        g = torch.Generator(device=cuda).manual_seed(H + bf16)
        for it in range(3):  # tags advance: every message must be taken, none twice
            msg = torch.empty(H + nhdr, device=cuda)
            msg[:H] = torch.randn(H, device=cuda, generator=g) * (10.0 ** (it - 1))
            hdr = torch.arange(nhdr, dtype=torch.int32, device=cuda) * 7919 + it
            msg[H:] = hdr.view(torch.float32)
            out = torch.full_like(msg, float("nan"))
            hop.send(msg, H, nhdr, bf16, _Self(inbox), sseq)
            hop.recv(inbox, out, H, nhdr, bf16, rseq, err, timeout_s=5.0)
            torch.cuda.synchronize()
            assert int(err.item()) == 0
            want = msg[:H].to(torch.bfloat16).float() if bf16 else msg[:H]
            assert torch.equal(out[:H], want), (it, (out[:H] - want).abs().max())
            assert torch.equal(out[H:].view(torch.int32), hdr)
            assert int(sseq.item()) == int(rseq.item()) == it + 1
    finally:
        inbox.close()


def test_hop_recv_times_out_with_error_word(cuda):
    """No sender: the receive gives up after its bound and raises the error word."""
    from cake_amd.parallel import hop
    H, nhdr = 128, 4
    inbox = hop.Inbox(hop.hop_words(H, nhdr, False))
    try:
        rseq = torch.zeros(1, dtype=torch.int32, device=cuda)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        out = torch.zeros(H + nhdr, device=cuda)
        hop.recv(inbox, out, H, nhdr, False, rseq, err, timeout_s=0.05)
        torch.cuda.synchronize()
        assert int(err.item()) == 1
    finally:
        inbox.close()


# ---------------------------------------------------------------------------
# small hops: special values, no header, less than one trip of the 512-thread loop
# ---------------------------------------------------------------------------

INVALID = 1   # hipErrorInvalidValue


def _special_payload(H, it):
    """H f32 values: signed zeros, infinities, NaN, f32 subnormals, a value above bf16's
    largest (rounds to inf there), ties between two bf16 values that round down to even
    (1 + 2^-8, 2^-126 + 2^-134) and up to even (1 + 3 * 2^-8, largest-bf16-subnormal tie), then
    random values; rotated by the message number so every slot sees several of them."""
    sp = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-40,
                       1.1754942e-38, 3.4e38, -3.4e38, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                       -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 2.0 ** -126 + 2.0 ** -134,
                       2.0 ** -126 - 2.0 ** -134, 65504.0, 3.3895314e38], dtype=torch.float32)
    g = torch.Generator().manual_seed(H * 7 + it)
    v = torch.cat([sp.roll(it * 5), torch.randn(max(0, H - sp.numel()), generator=g) * 100.0])
    return v[:H].clone()


@pytest.mark.parametrize("H,nhdr,bf16", [(1, 0, False), (2, 0, False), (2, 0, True), (514, 3, False),
                                         (514, 3, True), (1026, 1, False), (1026, 1, True)])
def test_hop_small_and_special(cuda, H, nhdr, bf16):
    """One and two words, no header, and sizes just past one and two trips of the 512-thread
    loop; special values.  f32 bit-exact (NaN payload included), bf16 the bits of
    .to(torch.bfloat16) (NaN for NaN); the words behind the message stay."""
    from cake_amd.parallel import hop
    inbox = hop.Inbox(hop.hop_words(H, nhdr, bf16))
    try:
        sseq = torch.zeros(1, dtype=torch.int32, device=cuda)
        rseq = torch.zeros(1, dtype=torch.int32, device=cuda)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        for it in range(3):
            pay = _special_payload(H, it)
            hdr = torch.arange(nhdr, dtype=torch.int32) * 7919 - it
            msg = torch.cat([pay, hdr.view(torch.float32)]).to(cuda)
            buf = torch.full((H + nhdr + 32,), 12345.678, device=cuda)
            out = buf[:H + nhdr]
            hop.send(msg, H, nhdr, bf16, _Self(inbox), sseq)
            hop.recv(inbox, out, H, nhdr, bf16, rseq, err, timeout_s=5.0)
            torch.cuda.synchronize()
            assert int(err.item()) == 0
            got = out.cpu()
            if bf16:
                want = pay.to(torch.bfloat16)
                nan = want.isnan()
                g16 = got[:H].to(torch.bfloat16)
                assert torch.equal(g16.float()[~nan], got[:H][~nan])       # bf16 values, exactly
                assert torch.equal(got[:H].isnan(), nan)
                assert torch.equal(g16.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), it
            else:
                assert torch.equal(got[:H].view(torch.int32), pay.view(torch.int32)), it
            assert torch.equal(got[H:].view(torch.int32), hdr)
            assert bool((buf[H + nhdr:] == torch.tensor(12345.678, device=cuda)).all())
            assert int(sseq.item()) == int(rseq.item()) == it + 1
    finally:
        inbox.close()


def test_hop_refusals(cuda):
    from cake_amd.ops._lib import kernels
    from cake_amd.parallel import hop
    lib = kernels()
    st = torch.cuda.current_stream().cuda_stream
    inbox = hop.Inbox(64)
    try:
        msg = torch.zeros(64, device=cuda)
        seq = torch.zeros(1, dtype=torch.int32, device=cuda)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        m, s, e = msg.data_ptr(), seq.data_ptr(), err.data_ptr()
        for H, nhdr, bf16 in [(3, 0, 1), (1, 2, 1), (0, 4, 0), (0, 4, 1), (-2, 0, 0), (4, -1, 0), (4, -1, 1)]:
            assert lib.cake_hop_send(m, H, nhdr, bf16, inbox.ptr, s, st) == INVALID, (H, nhdr, bf16)
            assert lib.cake_hop_recv(inbox.ptr, H, nhdr, bf16, m, s, e, 1.0, st) == INVALID, (H, nhdr, bf16)
        for t in (0.0, -1.0):
            assert lib.cake_hop_recv(inbox.ptr, 4, 0, 0, m, s, e, t, st) == INVALID
        torch.cuda.synchronize()
        assert int(seq.item()) == 0 and int(err.item()) == 0 and not bool(msg.any())
    finally:
        inbox.close()


# ---------------------------------------------------------------------------
# bulk hops
# ---------------------------------------------------------------------------

CHUNKS = [1, 1023, 1024, 1025, 4 * 256 * 7 + 5]     # 16-byte chunks per segment: below, at and
                                                    # past one block's unrolled trip; 8 blocks
                                                    # with an unrolled trip and a tail


def _bulk_pair(nbytes, dev):
    """A bulk channel into this process's own inbox."""
    from cake_amd.parallel import hop
    inbox = hop.BulkInbox(nbytes, dev)
    peer = hop.BulkPeer.__new__(hop.BulkPeer)        # no IPC mapping: the inbox itself
    peer.nbytes, peer.peer = inbox.nbytes, _Self(inbox.box)
    peer.seq = torch.zeros(1, dtype=torch.int32, device=dev)
    peer.count = torch.zeros(1, dtype=torch.int32, device=dev)
    return inbox, peer


def _segments(sizes16, gen, dev):
    return [torch.randint(-2 ** 31, 2 ** 31 - 1, (4 * c,), generator=gen, dtype=torch.int32).to(dev)
            for c in sizes16]


def _layout(sizes16, order, gap16):
    """Byte offsets of the segments laid out in `order` with gap16 free chunks after each."""
    offs, at = [0] * len(sizes16), 0
    for k in order:
        offs[k] = at * 16
        at += sizes16[k] + gap16
    return offs, at * 16


def _bulk_check(inbox, peer, image, segs, offs, number, dst):
    """After message `number`: the received buffer is the inbox image with the segments at
    their offsets (everything else as the previous message left it), the arrival counter is
    back at 0 and both sequence words are the message number."""
    for t, o in zip(segs, offs):
        image[o // 4:o // 4 + t.numel()] = t
    torch.cuda.synchronize()
    assert not inbox.error()
    assert torch.equal(dst, image), f"message {number}"
    assert int(peer.count.item()) == 0
    assert int(peer.seq.item()) == int(inbox.seq.item()) == number


def test_bulk_hop_segments(cuda):
    """Three messages in a row on one channel: 3 segments at out-of-order offsets with gaps,
    1 segment, 32 segments; every segment size of CHUNKS."""
    g = torch.Generator().manual_seed(5)
    sizes32 = [CHUNKS[k % 5] for k in range(32)]
    order32 = torch.randperm(32, generator=g).tolist()
    offs32, total = _layout(sizes32, order32, 3)
    inbox, peer = _bulk_pair(total, cuda)
    try:
        image = torch.zeros(inbox.nbytes // 4, dtype=torch.int32, device=cuda)   # a new inbox is zero
        dst = torch.full_like(image, 0x5A5A5A5A)
        plans = [([CHUNKS[1], CHUNKS[0], CHUNKS[4]], [2, 0, 1], 7), ([CHUNKS[3]], [0], 0),
                 (sizes32, order32, 3)]
        for number, (sizes, order, gap) in enumerate(plans, 1):
            offs, end = _layout(sizes, order, gap)
            assert end <= inbox.nbytes
            if number == 2:
                offs = [16 * 5]                       # inside message 1's first segment
            segs = _segments(sizes, g, cuda)
            peer.send(segs, offs)
            inbox.recv(dst, timeout_s=5.0)
            _bulk_check(inbox, peer, image, segs, offs, number, dst)
            if number == 1:   # the gap behind its first segment: still the zeros of a new inbox
                gap = slice((offs[2] + sizes[2] * 16) // 4, offs[0] // 4)
                assert gap.stop - gap.start == 7 * 4 and not bool(dst[gap].any())
    finally:
        inbox.close()


def test_bulk_hop_large_segment_with_a_small_one(cuda):
    """24 MiB (more than four trips of the 1024-block grid: the unrolled loop and its tail)
    and a one-chunk segment in one launch; the large one sits past the small one and a gap."""
    big = 24 * 2 ** 20
    inbox, peer = _bulk_pair(big + 64, cuda)
    try:
        g = torch.Generator().manual_seed(6)
        image = torch.zeros(inbox.nbytes // 4, dtype=torch.int32, device=cuda)
        dst = torch.full_like(image, 0x5A5A5A5A)
        segs = _segments([big // 16, 1], g, cuda)
        offs = [64, 16]
        peer.send(segs, offs)
        inbox.recv(dst, timeout_s=5.0)
        _bulk_check(inbox, peer, image, segs, offs, 1, dst)
        assert not bool(dst[:4].any()) and not bool(dst[8:16].any())      # the gaps: zeros
    finally:
        inbox.close()


def test_bulk_hop_graph_replay(cuda):
    """The same send and receive captured in one graph on one stream: each replay delivers
    the bytes its sources hold at that moment, and the tags stay in step."""
    sizes, order = [CHUNKS[4], CHUNKS[0], CHUNKS[3]], [1, 2, 0]
    offs, total = _layout(sizes, order, 2)
    inbox, peer = _bulk_pair(total, cuda)
    try:
        g = torch.Generator().manual_seed(7)
        image = torch.zeros(inbox.nbytes // 4, dtype=torch.int32, device=cuda)
        dst = torch.full_like(image, 0x5A5A5A5A)
        segs = _segments(sizes, g, cuda)
        peer.send(segs, offs)                         # message 1, outside the graph
        inbox.recv(dst, timeout_s=5.0)
        _bulk_check(inbox, peer, image, segs, offs, 1, dst)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            peer.send(segs, offs)
            inbox.recv(dst, timeout_s=5.0)
        for number in (2, 3, 4):
            for t, new in zip(segs, _segments(sizes, g, cuda)):
                t.copy_(new)
            dst.fill_(0x5A5A5A5A)
            graph.replay()
            _bulk_check(inbox, peer, image, segs, offs, number, dst)
    finally:
        inbox.close()


def test_bulk_hop_refusals(cuda):
    import ctypes as C
    from cake_amd.ops._lib import kernels
    lib = kernels()
    st = torch.cuda.current_stream().cuda_stream
    rx = 4096
    inbox, peer = _bulk_pair(rx, cuda)
    try:
        src = torch.zeros(2048, dtype=torch.int32, device=cuda)
        dst = torch.zeros(rx // 4 + 8, dtype=torch.int32, device=cuda)
        s, c = peer.seq.data_ptr(), peer.count.data_ptr()

        def send(ptrs, sizes, offs, nseg, rx_bytes=rx):
            n = len(ptrs)
            return lib.cake_bulk_send((C.c_void_p * n)(*ptrs), (C.c_uint64 * n)(*sizes),
                                      (C.c_uint64 * n)(*offs), nseg, inbox.box.ptr, rx_bytes, s, c, st)
        p = src.data_ptr()
        assert send([p], [64], [0], 0) == INVALID                           # no segment
        assert send([p] * 33, [16] * 33, [16 * k for k in range(33)], 33) == INVALID
        assert send([p], [40], [0], 1) == INVALID                           # size % 16
        assert send([p], [64], [8], 1) == INVALID                           # offset % 16
        assert send([p + 4], [64], [0], 1) == INVALID                       # misaligned source
        assert send([p], [64], [rx - 48], 1) == INVALID                     # past the inbox
        assert send([p, p], [64, rx], [0, 16], 2) == INVALID                # its second segment too
        assert send([p], [64], [0], 1, rx_bytes=2 ** 31) == INVALID
        assert send([p], [64], [0], 1, rx_bytes=rx + 8) == INVALID
        e = inbox.err.data_ptr()
        assert lib.cake_bulk_recv(inbox.box.ptr, rx, dst.data_ptr() + 4, inbox.seq.data_ptr(), e, 1.0, st) == INVALID
        assert lib.cake_bulk_recv(inbox.box.ptr, rx, dst.data_ptr(), inbox.seq.data_ptr(), e, 0.0, st) == INVALID
        assert lib.cake_bulk_recv(inbox.box.ptr, rx + 8, dst.data_ptr(), inbox.seq.data_ptr(), e, 1.0, st) == INVALID
        torch.cuda.synchronize()
        assert int(peer.seq.item()) == int(inbox.seq.item()) == int(peer.count.item()) == 0
        assert not inbox.error() and not bool(dst.any())
        with pytest.raises(ValueError):
            inbox.recv(dst[1:], timeout_s=1.0)
        with pytest.raises(ValueError):
            peer.send([src[:16]] * 33, [0] * 33)
    finally:
        inbox.close()
