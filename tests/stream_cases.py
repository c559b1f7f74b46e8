"""The seeded, GPU-free batch sequences of tests/test_gpu_stream.py (`TextDetector.detect_stream` against the unpipelined
`detect_batch`, batch for batch), checked without a GPU in tests/test_stream_cases.py.  Every sequence is a list of
`(kind, pages)`: `pages` a list of BGR uint8 (H,W,3) numpy arrays, `kind` one of

    blank    pages of ONE flat grey, another grey for every blank batch of a sequence -- nothing to detect;
    dense    `synth.text_like_page` pages, a seed of its own for every page of a sequence;
    sparse   a flat page with a few patches cut out of a text-like page (`patch_page`): little for the tail to do.

The sequences are longer than every ring of the pipeline (`detect_stream`'s `depth` batches in flight, `_stage`'s pinned slots
per loader thread): tests/test_stream_cases.py reads both sizes from detector.py and holds every sequence against them.

`stream_checkpoint()` is the checkpoint the stream tests run: seeded random weights answer a flat page and a page of text
alike (the Detect head's objectness varies by 0.02 over ALL pages, the DB head's map is over its threshold on some part of any
page; measured with the oracle network: 6 .. 41 blocks on flat pages whatever their colour, `make_checkpoint` and
`make_blob_checkpoint` alike).  A stream whose batches all give about the same answer cannot show a batch that was read too
early or too late, so the blob checkpoint's last DB layer is sharpened around a logit that no flat page of grey 0 .. 169 reaches
and its Detect head is closed: blocks then come from the DB head's text lines alone (`group_output`'s scattered lines), none on
a blank page, around a hundred on a dense one at 256 x 256.
"""
import math

import numpy as np

BLANK, DENSE, SPARSE = "blank", "dense", "sparse"

# ------------------------------------------------------------------------------------------------------------ the pages

BLANK_GREYS = tuple(range(8, 170, 12))          # 14 greys; `stream_checkpoint` is calibrated for flat greys below 170


def blank_page(shape, k):
    """The flat page of blank batch number `k` of a sequence."""
    return np.full(tuple(shape) + (3,), BLANK_GREYS[k % len(BLANK_GREYS)], np.uint8)


def dense_page(shape, seed, n_blocks=8):
    from conftest import pkg
    return pkg().synth.text_like_page(tuple(shape), int(seed), n_blocks=n_blocks)


def patch_page(shape, seed, n_patches=2, patch=96, grey=56):
    """A flat dark page with `n_patches` patch x patch pieces of a text-like page pasted at seeded places."""
    h, w = shape
    rng = np.random.RandomState(seed)
    src = dense_page((max(h, 256), max(w, 256)), 50000 + seed, n_blocks=12)
    page = np.full((h, w, 3), grey, np.uint8)
    for _ in range(n_patches):
        sy, sx = int(rng.randint(0, src.shape[0] - patch + 1)), int(rng.randint(0, src.shape[1] - patch + 1))
        y, x = int(rng.randint(0, h - patch + 1)), int(rng.randint(0, w - patch + 1))
        page[y: y + patch, x: x + patch] = src[sy: sy + patch, sx: sx + patch]
    return page


# -------------------------------------------------------------------------------------------------------- the sequences

def alternating(n=26, pages=3, size=256, seed=1000, n_blocks=8):
    """Batch k is blank for even k and dense for odd k, every page size x size: the caching allocator hands each forward the
    blocks the one before it freed, and a batch that reads its neighbour's bytes reads another kind of page.  26 batches take
    `depth` = 4 round six times and the 2 x 3 pinned slots of two loader threads four times."""
    out = []
    for k in range(n):
        if k % 2 == 0:
            out.append((BLANK, [blank_page((size, size), k // 2) for _ in range(pages)]))
        else:
            out.append((DENSE, [dense_page((size, size), seed + 16 * k + j, n_blocks) for j in range(pages)]))
    return out


MIXED_SHAPES = ((144, 200), (300, 212), (200, 180))     # letterboxed up and down at 256; within (144, 200) .. (300, 212)


def mixed_sizes(n=20, size=256, seed=3000):
    """A cycle of four batches: 3 pages of size x size (staged back to back: `_as_batch` returns a view of the upload), 3 pages
    of three other shapes (letterboxed: `torch.stack` copies), 2 pages, 5 pages (a pinned slot made for 3 pages is too small:
    it is allocated again, larger, in the middle of the stream).  Every page is dense with a seed of its own, except the
    middle page of every 5-page batch, which is blank."""
    out = []
    for k in range(n):
        shapes = ([(size, size)] * 3, list(MIXED_SHAPES), [(size, size)] * 2, [(size, size)] * 5)[k % 4]
        pages = [dense_page(sh, seed + 16 * k + j, 6) for j, sh in enumerate(shapes)]
        if k % 4 == 3:
            pages[2] = blank_page((size, size), k // 4)
        out.append((DENSE, pages))
    return out


# What tests/test_gpu_stream.py runs for the two lapping cases (its docstring has the times measured for them).
FORWARD_HEAVY = dict(n=12, pages=8, size=1024)
TAIL_HEAVY = dict(n=12, pages=4, size=512, n_blocks=16)


def forward_heavy(n=FORWARD_HEAVY["n"], pages=FORWARD_HEAVY["pages"], size=FORWARD_HEAVY["size"], seed=5000):
    """Blank batches alternating with batches of pages of two patches: a long forward, next to nothing for the tail."""
    out = []
    for k in range(n):
        if k % 2 == 0:
            out.append((BLANK, [blank_page((size, size), k // 2) for _ in range(pages)]))
        else:
            out.append((SPARSE, [patch_page((size, size), seed + 16 * k + j) for j in range(pages)]))
    return out


def tail_heavy(n=TAIL_HEAVY["n"], pages=TAIL_HEAVY["pages"], size=TAIL_HEAVY["size"], n_blocks=TAIL_HEAVY["n_blocks"], seed=7000):
    """Dense pages only, a seed of its own each: a short forward and a long tail (run with one worker, `refine_mode` 1 and
    `keep_undetected_mask`)."""
    return [(DENSE, [dense_page((size, size), seed + 16 * k + j, n_blocks) for j in range(pages)]) for k in range(n)]


SEQUENCES = {"alternating": alternating, "mixed_sizes": mixed_sizes, "forward_heavy": forward_heavy, "tail_heavy": tail_heavy}


# ------------------------------------------------------------------------------------------------------- the checkpoint

DB_GAIN, DB_PIVOT = 4.0, -0.6


def stream_checkpoint():
    """`synth.make_blob_checkpoint(0)` with (1) the DB head's final logit z replaced by DB_GAIN * (z - DB_PIVOT) + logit(0.3):
    the oracle network's z stays below -0.84 on every flat grey page of `BLANK_GREYS` (and on flat pages of any colour with
    channels below 170), so such a page has probability < 0.21 everywhere -- no pixel over the 0.3 threshold, no text line --
    while a twentieth of a text-like page lies above -0.26, that is above 0.62; (2) every objectness bias of the Detect head
    lowered by 20: no page has a candidate box (the head cannot tell pages apart, see the module docstring)."""
    from conftest import pkg
    ck = pkg().synth.make_blob_checkpoint(0)
    td = ck["text_det"]
    b = float(td["binarize.6.bias"])
    td["binarize.6.weight"] = td["binarize.6.weight"] * DB_GAIN
    td["binarize.6.bias"] = td["binarize.6.bias"].new_tensor([DB_GAIN * (b - DB_PIVOT) + math.log(0.3 / 0.7)])
    w8 = ck["blk_det"]["weights"]
    det_i = max(int(k.split(".")[1]) for k in w8 if k.endswith(".anchors"))
    for j in range(3):
        bias = w8[f"model.{det_i}.m.{j}.bias"]
        bias.view(-1, bias.numel() // 3)[:, 4] -= 20.0
    return ck
