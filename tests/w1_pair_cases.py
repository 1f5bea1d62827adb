"""The conv_w1 cases that pin the producers' item shape (one lane = two adjacent column pairs, six pixel loads for eight): shared by
tools/probes/w1_capture_bits.py (which recorded tests/golden/w1_parent_bits.npz with the half-row items of the commit before), the CPU
tier (tests/test_emu_w1_pair_lanes.py) and the GPU tier (tests/test_gpu_w1_pair_lanes.py).  The smallest shapes that reach each way the
lane mapping can go wrong: (name, (N, H, W, Cin, Cout, reflect), keywords of op_cases.conv_w1_case, chunk sizes, error line or None = REL)."""
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w1_parent_bits.npz")

CASES = (
    # both image borders inside one tile (columns -1 and 32 reflected); one slab: the only period's second slab is all zeros
    ("borders_one_slab", (1, 4, 32, 16, 64, True), dict(), (1,), None),
    # two column tiles: a halo pixel of the neighbouring tile; a zero-padded pixel shared by a lane's two pairs is re-zeroed in both
    ("zpad_two_tiles", (1, 4, 64, 32, 64, False), dict(norm=True), (1,), None),
    # several tiles and images, an odd slab count with a table per image
    ("zpad_images_odd", (2, 8, 64, 48, 64, False), dict(norm=True), (1,), None),
    ("reflect_odd_norelu", (1, 4, 32, 80, 64, True), dict(norm=True, relu=False), (1,), None),
    # the scaled split of the raw no-ReLU path
    ("raw_scaled", (1, 4, 32, 32, 64, True), dict(scale=300.0), (1,), None),
    # chunks that cross from one image into the next: the second table, the next tile's offsets
    ("chunks_reflect", (6, 16, 32, 128, 64, True), dict(norm=True), (1, 3), None),
    ("chunks_zpad_norelu", (4, 16, 32, 128, 64, False), dict(norm=True, relu=False), (1, 2), None),
    # the hot path of the chunk kernel (five periods and more: steady loop, last period, crossing, next tile) on a raw input without ReLU
    ("raw_norelu_six_periods", (4, 16, 32, 192, 64, True), dict(), (1, 2), None),
    # the same path with an odd slab count (the last period's second slab masked where it is fetched) under zero padding + IN + ReLU: the
    # re-zeroing of a shared padded pixel in the chunk kernel
    ("zpad_odd_five_periods", (4, 16, 32, 144, 64, False), dict(norm=True), (1, 2), None),
    # bf16 operands: the one-tile kernel's single plane
    ("bf16_one_tile", (1, 4, 32, 32, 64, True), dict(norm=True, nprod=1), (1,), 2e-2),
)


LIMIT = 1000 * 1024          # a committed file stays under 1 MiB: the record is written in parts (w1_parent_bits.npz, .part2.npz, ...)


def part_path(i):
    return GOLDEN if i == 0 else GOLDEN.replace(".npz", f".part{i + 1}.npz")


def load_golden():
    """{case name: NHWC output of the commit before} from every part of the record (one array per case: its chunk sizes gave equal bits)"""
    import numpy as np
    rec, i = {}, 0
    while os.path.exists(part_path(i)):
        with np.load(part_path(i)) as z:
            rec.update({k: z[k] for k in z.files})
        i += 1
    return rec


def outputs(oc, lib, dev, name, args, kw, chunks):
    """{chunk: NHWC output} of one case"""
    return {c: oc.conv_w1_case(lib, dev, *args, chunk=c, return_output=True, **kw) for c in chunks}
