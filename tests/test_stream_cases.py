"""The batch sequences of the stream tests (tests/stream_cases.py) checked WITHOUT a GPU: the same call gives the same bytes,
every stream tests/test_gpu_stream.py runs is longer than the rings of the pipeline it goes through -- the sizes of those rings
read from detector.py, so a change there is reported here --, consecutive batches share no page, and the checkpoint of the stream
tests tells a blank page from a dense one (oracle network and oracle tail on the first batches)."""
import inspect
import re

import numpy as np
import pytest

import stream_cases as SC
from conftest import pkg


def _bytes(seq):
    return b"|".join(kind.encode() + b":" + b",".join(repr(p.shape).encode() + p.tobytes() for p in pages) for kind, pages in seq)


@pytest.mark.parametrize("name", sorted(SC.SEQUENCES))
def test_sequences_are_reproducible_byte_for_byte(name):
    a, b = SC.SEQUENCES[name](), SC.SEQUENCES[name]()
    assert _bytes(a) == _bytes(b)
    assert all(p.dtype == np.uint8 and p.ndim == 3 and p.shape[2] == 3 and p.flags.c_contiguous for _, pages in a for p in pages)


def test_a_seed_changes_the_dense_pages_only():
    a, b = SC.alternating(4), SC.alternating(4, seed=1001)
    assert _bytes(a[::2]) == _bytes(b[::2]) and all(_bytes([x]) != _bytes([y]) for x, y in zip(a[1::2], b[1::2]))


def pipeline_rings():
    """(pinned slots per loader thread, default `depth`, default `loaders`) as detector.py has them: the literal of `_stage`'s
    ring and the defaults of `detect_stream`."""
    det = pkg().detector.TextDetector
    ring = re.findall(r"if len\(tl\.ring\) < (\d+):", inspect.getsource(det._stage))
    assert len(ring) == 1, "the pinned ring of TextDetector._stage is no longer `if len(tl.ring) < N:` -- tell this test its size"
    par = inspect.signature(det.detect_stream).parameters
    return int(ring[0]), par["depth"].default, par["loaders"].default


def test_ring_sizes_are_the_ones_the_sequences_were_made_for():
    """`alternating`'s 26 batches are six rounds of depth 4 and four rounds of 2 x 3 pinned slots: if detector.py changes either
    size, this fails and the sequence lengths (and the runs of tests/test_gpu_stream.py) want another look."""
    assert pipeline_rings() == (3, 4, 2)


def test_every_stream_is_longer_than_depth_plus_the_pinned_slots_of_its_loaders():
    import test_gpu_stream as G
    ring, depth0, loaders0 = pipeline_rings()
    assert len(G.STREAMS) >= 20
    for name, kw in G.STREAMS:
        n = G.BOOKKEEPING["n"] if name == "stubs" else len(SC.SEQUENCES[name]())
        depth, loaders = kw.get("depth", depth0), kw.get("loaders", loaders0)
        assert n > depth + ring * loaders, (name, kw, n)
    assert len(SC.alternating()) >= 6 * depth0 and len(SC.alternating()) >= 4 * ring * loaders0
    # the run that stages more batches ahead than a loader has slots, and the one that waits for nothing in flight
    assert any(kw.get("depth", depth0) > ring and kw.get("loaders") == 2 for _, kw in G.STREAMS)
    assert any(kw.get("depth") == 1 for _, kw in G.STREAMS)


def test_consecutive_batches_share_no_page():
    for name in ("alternating", "forward_heavy", "tail_heavy", "mixed_sizes"):
        seq = SC.SEQUENCES[name]()
        for (ka, a), (kb, b) in zip(seq, seq[1:]):
            assert not {p.tobytes() for p in a} & {p.tobytes() for p in b}, name
    alt = SC.alternating()
    assert [k for k, _ in alt] == [SC.BLANK, SC.DENSE] * 13 and all(len(p) == 3 for _, p in alt)
    blanks = [p[0] for k, p in alt if k == SC.BLANK]
    assert all((p == p[0, 0, 0]).all() for p in blanks) and len({int(p[0, 0, 0]) for p in blanks}) == 13    # a grey per batch
    assert max(int(p[0, 0, 0]) for p in blanks) < 170                     # what `stream_checkpoint` is calibrated for
    assert len({p.tobytes() for k, pages in alt if k == SC.DENSE for p in pages}) == 39        # a seed per page and batch


def test_mixed_sizes_changes_shapes_page_counts_and_the_staged_bytes():
    seq = SC.mixed_sizes()
    assert len(seq) == 20
    counts = [len(p) for _, p in seq]
    assert counts[:4] == [3, 3, 2, 5] and counts == counts[:4] * 5
    for k, (_, pages) in enumerate(seq):
        shapes = [p.shape[:2] for p in pages]
        if k % 4 == 1:
            assert len(set(shapes)) == 3 and (256, 256) not in shapes
            assert all(144 <= h <= 300 and 180 <= w <= 212 for h, w in shapes)
        else:
            assert set(shapes) == {(256, 256)}                            # one size: staged back to back, batched as a view
    staged = [sum(p.size for p in pages) for _, pages in seq]
    assert max(staged[:3]) < staged[3]                                    # the 5-page batch outgrows every slot made before it


def test_lapping_sequences_are_twelve_batches_within_the_cap():
    for name, spec in (("forward_heavy", SC.FORWARD_HEAVY), ("tail_heavy", SC.TAIL_HEAVY)):
        seq = SC.SEQUENCES[name]()
        assert len(seq) == 12 and all(len(p) == spec["pages"] and p[0].shape == (spec["size"], spec["size"], 3) for _, p in seq)
        assert spec["pages"] <= 8 and spec["size"] <= 1024
    assert [k for k, _ in SC.forward_heavy()] == [SC.BLANK, SC.SPARSE] * 6
    assert {k for k, _ in SC.tail_heavy()} == {SC.DENSE}


def test_stream_checkpoint_tells_blank_pages_from_dense_ones():
    """Oracle network + oracle tail on the first pages of `alternating` and `forward_heavy` (measured over all of them: 0 blocks
    and an all-zero refined mask on every blank page, 102 .. 135 blocks on the dense pages, 13 .. 39 on the sparse ones)."""
    import torch
    from oracle import postproc_ref as R
    from oracle.net_ref import OracleNet
    net = OracleNet(SC.stream_checkpoint())

    def run(page):
        x = torch.from_numpy(np.ascontiguousarray(page.transpose(2, 0, 1)[None])).float() / 255
        blks, mask, lines = net(x)
        assert float(blks[..., 4].max()) < 0.4                            # the Detect head is closed
        return R.detector_tail(page, blks.numpy(), mask.numpy(), lines.numpy(), input_size=page.shape[:2]), float(lines[0, 0].max())

    alt = SC.alternating(2)
    (_, refined, blocks), top = run(alt[0][1][0])
    assert blocks == [] and not refined.any() and top < 0.25
    dense = [run(p)[0] for p in alt[1][1]]
    assert all(len(r[2]) >= 6 for r in dense) and any(r[1].any() for r in dense)
    (_, refined, blocks), top = run(SC.blank_page((256, 256), len(SC.BLANK_GREYS) - 1))    # the lightest grey
    assert blocks == [] and not refined.any() and top < 0.25
    sparse = run(SC.forward_heavy(2, 1, 512)[1][1][0])[0]
    assert len(sparse[2]) >= 6
