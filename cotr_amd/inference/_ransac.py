"""What only the wrappers of the RANSAC estimators share (guided, homography, essential, pnp, rigid3d): the pair of point
sets, the threshold / confidence / max_iters check, the seed and the tensors of one estimator call, in one wording for all of
them.  Built on ``_args``, where the rules every wrapper shares live; ``_args`` imports nothing from here."""
from . import _args
from ._args import F64, I32, MAX_POINTS, U8  # noqa: F401 (MAX_POINTS: the estimators' limit, read as _ransac.MAX_POINTS)

MAX_ITERS = 1 << 16


def pairs(points1, points2, least, too_few):
    """-> (points1, points2, n) as [n, 2] float64 tensors; ``too_few``: the message below ``least`` correspondences, the
    model's own"""
    p1, p2 = _args.points(points1, 'points1'), _args.points(points2, 'points2')
    _args.count_pairs(p1.shape[0], p2.shape[0], least, too_few, 'points1', 'points2')
    return p1, p2, p1.shape[0]


def check_ransac(threshold, confidence, max_iters, most_iters=MAX_ITERS):
    _args.check_int_range('max_iters', max_iters, 1, most_iters, integer=False)
    _args.check_positive('the RANSAC threshold', threshold)
    if not 0 < confidence < 1:
        raise ValueError(f'confidence must be in (0, 1), got {confidence}')


def seed64(seed):
    return int(seed) & ((1 << 64) - 1)


def outputs(lib, scratch_bytes, n, max_iters, model, slots, info_len, hyp_key, hypotheses, device):
    """the tensors of one estimator call -> (scratch uint8, result float64 [9], mask uint8 [n], dict(info int32 [info_len]) with,
    when ``hypotheses``, samples int32 [max_iters, model], ``hyp_key`` float64 [slots * max_iters, 9] and hyp_count int32
    [slots * max_iters]).  scratch_bytes: the name of the library's ``*_scratch_bytes`` function."""
    scratch, _ = _args.scratch(lib, scratch_bytes, n, max_iters, device=device)
    result, mask, info = _args.empty(device, (9, F64), (n, U8), (info_len, I32))
    out = dict(info=info)
    if hypotheses:
        out['samples'], out[hyp_key], out['hyp_count'] = _args.empty(device, ((max_iters, model), I32), ((slots * max_iters, 9), F64),
                                                                     (slots * max_iters, I32))
    return scratch, result, mask, out
