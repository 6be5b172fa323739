"""Executable statement of the contract of vsc_match_maps_f32 (include/vsc_hip.h) in numpy, with the summation order of the
view score spelled out.  Test helper only: the GPU tests compare the kernels with it bit for bit, the CPU tests compare it
with src.matching._best_view + MatchClassifyDataset / MatchRefineDataset; the project never runs it in place of the kernels."""
import numpy as np

TOP_ROWS = 10      # VSC_MATCH_TOP_ROWS


def view_score(row_max):
    """fl(S / c) of the c = min(10, len) largest values, S summed in numpy's pairwise order, everything in float32."""
    a = np.sort(np.asarray(row_max, np.float32))[-TOP_ROWS:]
    c = len(a)
    f = np.float32
    if c < 8:
        s = a[0]
        for k in range(1, c):
            s = f(s + a[k])
    else:
        s = f(f(f(a[0] + a[1]) + f(a[2] + a[3])) + f(f(a[4] + a[5]) + f(a[6] + a[7])))
        for k in range(8, c):
            s = f(s + a[k])
    return f(s / f(c))


def check_item(q_rows, r_rows, frames):
    """The launcher's refusals (beyond "inside the buffer")."""
    if frames < 1:
        raise ValueError(f"{frames} frames per view")
    if q_rows > frames:
        if r_rows < 1:
            raise ValueError("a multi-view item without columns")
        if q_rows % frames:
            raise ValueError(f"ragged views: {q_rows} rows in views of {frames}")


def view_start(s, frames):
    """Start row of the first view whose score is strictly greater than every earlier one; 0 for a single-view item."""
    q_rows = s.shape[0]
    check_item(q_rows, s.shape[1], frames)
    if q_rows <= frames:
        return 0
    best, best_score = 0, None
    for start in range(0, q_rows, frames):
        m = np.full(frames, -np.inf, np.float32)
        for i in range(frames):
            m[i] = s[start + i].max()
        score = view_score(m)
        if best_score is None or score > best_score:
            best, best_score = start, score
    return best


def valid_hw(q_rows, r_rows, frames, resolution):
    return min(frames, q_rows, resolution), min(r_rows, resolution)


def match_maps(flat, items, resolution, with_transpose):
    """-> (view_start int32 [n], out float32 [n * (1 + with_transpose), R, R, 3])"""
    flat = np.asarray(flat, np.float32).reshape(-1)
    items = np.asarray(items, np.int64).reshape(-1, 4)
    R, slices = int(resolution), 2 if with_transpose else 1
    starts = np.zeros(len(items), np.int32)
    out = np.zeros((len(items) * slices, R, R, 3), np.float32)
    for p, (off, q_rows, r_rows, frames) in enumerate(items):
        if off < 0 or off + q_rows * r_rows > flat.size:
            raise ValueError(f"item {p} outside the {flat.size} similarities")
        s = flat[off:off + q_rows * r_rows].reshape(q_rows, r_rows)
        vs = starts[p] = view_start(s, frames)
        h, w = valid_hw(q_rows, r_rows, frames, R)
        out[p * slices, :h, :w, :] = s[vs:vs + h, :w, None]
        if with_transpose:
            out[p * slices + 1, :w, :h, :] = s[vs:vs + h, :w].T[:, :, None]
    return starts, out


def bits(x):
    """float32 array -> its uint32 bit patterns (everything here is compared exactly)"""
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
