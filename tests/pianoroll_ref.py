"""Seeded inputs of the piano-roll tests, shared with tools/make_pianoroll_golden.py: tests/golden/g14_pianoroll.npz stores only what
upstream's functions returned for them.  Nothing here needs a GPU."""
import numpy as np

POOL = np.array([0, 19, 20, 21, 254, 255], dtype=np.uint8)       # both sides of thresh = 20, and the top of the range

# name -> (seed, H, W, runs per row, noise pixels per row, rows used or None for all)
DECODE_CASES = {
    "strips128": (101, 128, 128, 3.0, 4.0, None),
    "strips640": (102, 640, 128, 3.0, 4.0, None),                # 5 strips: T = 640 crosses the separator at 512; flag restarts every 128
    "square": (103, 256, 256, 3.0, 4.0, None),
    "grid": (104, 2048, 2048, 6.0, 8.0, 40),                     # sparse: 40 of the 2048 image rows carry anything
}
PAINT_COLUMNS = 200


def make_image(seed, h, w, runs=3.0, noise=4.0, rows=None, green_r0=True):
    """uint8 [3,H,W]: per image row a few runs (a red pixel and a green tail, some tails without their red, some reds alone, runs that
    touch and runs that reach the last column), then single pixels whose channels come from POOL or are random.  With ``green_r0`` every
    pixel of class G gets r = 0 (the condition under which upstream's r + g equals g)."""
    rng = np.random.default_rng(seed)
    img = np.zeros((3, h, w), dtype=np.uint8)
    use = np.arange(h) if rows is None else np.sort(rng.choice(h, size=rows, replace=False))
    for y in use:
        for _ in range(rng.poisson(runs)):
            x0 = int(rng.integers(0, w))
            n = int(rng.integers(1, 24))
            val = int(rng.choice([21, 22, 60, 131, 254, 255, int(rng.integers(21, 256))]))
            kind = rng.random()
            x1 = min(w, x0 + n)
            if kind < 0.75:                                      # red onset + green tail
                img[:, y, x0] = (val, 0, 0)
                img[1, y, x0 + 1:x1] = val
            elif kind < 0.9:                                     # a tail without its onset
                img[1, y, x0:x1] = val
            else:                                                # white
                img[:, y, x0:x1] = val
        k = rng.poisson(noise)
        xs = rng.integers(0, w, size=k)
        for x in xs:
            px = np.where(rng.random(3) < 0.7, rng.choice(POOL, size=3), rng.integers(0, 256, size=3)).astype(np.uint8)
            img[:, y, x] = px
    if rows is None:                                             # the corners of the rule
        img[:, 5, :] = 0
        img[1, 5, :] = 200                                       # a full-width green row without a red
        img[:, 6, :] = 0
        img[1, 6, 1:] = 90
        img[0, 6, 0] = 90                                        # red at column 0, green to the last column
        img[:, 7, :] = 0
        img[0, 7, w - 1] = 255                                   # red in the last column
    if green_r0:
        r, g, b = img[0], img[1], img[2]
        img[0][(r < 20) & (g > 20) & (b < 20)] = 0
    return img


def decode_image(name):
    seed, h, w, runs, noise, rows = DECODE_CASES[name]
    return make_image(seed, h, w, runs, noise, rows)


def paint_notes():
    """int64 [n,4] (pitch, start, end, velocity) on PAINT_COLUMNS columns for the painter's golden: random notes, same-pitch overlaps in
    list order, and velocities 9, 10, 11 next to each other in every order (the thresholds of is_black / is_green).  No note of the pitch
    that reaches the last column starts at 0 (upstream wraps start - 1 = -1 round to the last column)."""
    rng = np.random.default_rng(7)
    notes = []
    for _ in range(150):
        s = int(rng.integers(1, PAINT_COLUMNS - 1))
        notes.append((int(rng.integers(20, 100)), s, min(PAINT_COLUMNS - 1, s + int(rng.integers(1, 30))), int(rng.integers(1, 128))))
    p = 100
    for a in (9, 10, 11):                                        # later list entries lie in FRONT, so their start - 1 zeroes nothing of a neighbour
        for c in (9, 10, 11):
            notes += [(p, 14, 18, c), (p, 10, 14, a)]            # columns 10..13 = a, 14..17 = c, column 9 zero
            p += 1
    notes += [(110, 0, 5, 64), (110, 5, 9, 64), (111, 0, 1, 10), (111, 1, 3, 11), (112, 0, 2, 11)]
    notes += [(113, 20, 60, 100), (113, 30, 40, 50), (113, 35, 80, 12), (113, 36, 37, 127)]      # overlaps: the last entry wins
    notes += [(114, 150, PAINT_COLUMNS, 90)]                     # the note that fixes the roll's length
    return np.asarray(notes, dtype=np.int64)
