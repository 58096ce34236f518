"""The seven entry points of the ELU + batch-norm tail (csrc/norm.hip) on the host: every refusal of their common preamble
(norm_enter: the dimension check with the row bound kNormMaxRows, then the workspace check for the five entries that need one) and of
the checks behind it, with null data pointers — each entry answers before it touches one — and sph3d_elu_bn_workspace against
tests/_norm_ref.py.  Every call here is refused: nothing is launched, no device is touched."""
import ctypes

import pytest

import _norm_ref as N

EINVAL, EWORKSPACE = -1, -2
BOUND = N.MAX_ROWS
_host = ctypes.create_string_buffer(8)
SOME = ctypes.addressof(_host)           # a non-null address no refused call may read: the checks only compare it with NULL


def _entries():
    """name -> call(R, C, **what is not NULL or 0), every other pointer NULL; NEED_WS: the entries that take a workspace"""
    from sph3d_gcn_amd import _lib
    l = _lib.lib()

    def forward(R, C, ws=None, wsb=0, training=1, running=None, **_):
        return l.sph3d_elu_bn_forward(R, C, None, None, None, running, running, 0.01, 1e-3, training, None, None, None, ws, wsb, None)

    def backward(R, C, ws=None, wsb=0, training=1, **_):
        return l.sph3d_elu_bn_backward(R, C, None, None, None, None, None, training, None, None, None, ws, wsb, None)

    def forward_partials(R, C, nblk=0, partial=None, **_):
        return l.sph3d_elu_bn_forward_partials(R, C, nblk, partial, None, None, None, None, None, 0.01, 1e-3, None, None, None, None)

    def forward_sums(R, C, ws=None, wsb=0, nblk=0, partial=None, sums=None, y=None, **_):
        return l.sph3d_elu_bn_forward_sums(R, C, nblk, partial, y, sums, ws, wsb, None)

    def forward_apply(R, C, sums=None, count=None, **_):
        return l.sph3d_elu_bn_forward_apply(R, C, sums, None, None, None, None, None, 0.01, 1e-3, None, None, None, count, None)

    def backward_sums(R, C, ws=None, wsb=0, sums=None, **_):
        return l.sph3d_elu_bn_backward_sums(R, C, None, None, None, None, None, None, sums, ws, wsb, None)

    def backward_apply(R, C, ws=None, wsb=0, sums=None, count=None, **_):
        return l.sph3d_elu_bn_backward_apply(R, C, sums, count, None, None, None, None, None, None, ws, wsb, None)

    e = dict(forward=forward, backward=backward, forward_partials=forward_partials, forward_sums=forward_sums,
             forward_apply=forward_apply, backward_sums=backward_sums, backward_apply=backward_apply)
    return l, e


NEED_WS = ("forward", "backward", "forward_sums", "backward_sums", "backward_apply")


@pytest.fixture(scope="module")
def lib_entries():
    return _entries()


def _refused(l, rc, status, text):
    msg = l.sph3d_last_error()
    assert rc == status and text in msg, (rc, status, text, msg)


def test_there_are_seven_entries_and_five_take_a_workspace(lib_entries):
    _, e = lib_entries
    assert len(e) == 7 and set(NEED_WS) < set(e)


@pytest.mark.parametrize("R,C", [(0, 4), (-1, 4), (8, 0), (8, 3), (8, 1028), (BOUND + 1, 4), (2 ** 31 - 1, 4), (-2 ** 31, 4)])
def test_bad_dimensions_are_refused_first(lib_entries, R, C):
    """before the workspace, before any pointer: all NULL, and with a workspace that would do"""
    l, e = lib_entries
    assert not N.supported(R, C)
    for name, call in e.items():
        _refused(l, call(R, C), EINVAL, b"sph3d_elu_bn_%s: needs 0<R<=%d" % (name.encode(), BOUND))
        _refused(l, call(R, C, ws=SOME, wsb=1 << 40, nblk=1, partial=SOME, sums=SOME, count=SOME), EINVAL, b"needs 0<R<=")


@pytest.mark.parametrize("R,C", [(BOUND, 4), (BOUND, 1024), (1, 4), (33, 12)])
def test_at_the_bound_the_dimension_check_passes_and_the_next_one_answers(lib_entries, R, C):
    l, e = lib_entries
    assert N.supported(R, C)
    for name in NEED_WS:
        _refused(l, e[name](R, C), EWORKSPACE, b"sph3d_elu_bn_%s: workspace 0 B < required %d B" % (name.encode(), N.workspace_bytes(R, C)))
    _refused(l, e["forward_apply"](R, C), EINVAL, b"sums / count is NULL")
    _refused(l, e["forward_partials"](R, C, nblk=0, partial=SOME), EINVAL, b"nblk=0")


@pytest.mark.parametrize("R,C", [(1, 4), (33, 12), (32769, 1024), (BOUND, 4)])
def test_workspace_short_or_null(lib_entries, R, C):
    l, e = lib_entries
    need = N.workspace_bytes(R, C)
    for name in NEED_WS:
        _refused(l, e[name](R, C, ws=SOME, wsb=need - 1, sums=SOME, count=SOME), EWORKSPACE, b"workspace %d B < required %d B" % (need - 1, need))
        _refused(l, e[name](R, C, ws=None, wsb=need, sums=SOME, count=SOME), EWORKSPACE, b"workspace")
    # with a supplied partial, forward_sums needs none: the next check answers
    _refused(l, e["forward_sums"](R, C, nblk=0, partial=SOME, sums=SOME), EINVAL, b"nblk=0 partial row blocks")
    _refused(l, e["forward_sums"](R, C, nblk=-1, partial=SOME, sums=SOME), EINVAL, b"nblk=-1 partial row blocks")


def test_null_sums_count_y_and_running_statistics(lib_entries):
    l, e = lib_entries
    R, C = 33, 12
    ok = dict(ws=SOME, wsb=N.workspace_bytes(R, C))
    _refused(l, e["forward_sums"](R, C, **ok), EINVAL, b"sums is NULL")
    _refused(l, e["forward_sums"](R, C, nblk=1, partial=SOME), EINVAL, b"sums is NULL")
    _refused(l, e["forward_sums"](R, C, sums=SOME, **ok), EINVAL, b"y is NULL")
    _refused(l, e["forward_apply"](R, C, sums=SOME), EINVAL, b"sums / count is NULL")
    _refused(l, e["forward_apply"](R, C, count=SOME), EINVAL, b"sums / count is NULL")
    _refused(l, e["backward_sums"](R, C, **ok), EINVAL, b"sums is NULL")
    _refused(l, e["backward_apply"](R, C, sums=SOME, **ok), EINVAL, b"sums / count is NULL")
    _refused(l, e["backward_apply"](R, C, count=SOME, **ok), EINVAL, b"sums / count is NULL")
    _refused(l, e["forward"](R, C, training=0, **ok), EINVAL, b"inference needs running statistics")
    _refused(l, e["forward_partials"](R, C, nblk=0, partial=SOME), EINVAL, b"nblk=0 partial row blocks")


@pytest.mark.parametrize("C", [4, 12, 1024])
@pytest.mark.parametrize("R", [1, 31, 32, 33, 32768, 32769, BOUND])
def test_workspace_size(lib_entries, R, C):
    l, _ = lib_entries
    assert l.sph3d_elu_bn_workspace(R, C) == N.workspace_bytes(R, C) == 4 * (min(1024, -(-R // 32)) * 2 * C + 2 * C)


def test_the_bound_is_the_one_the_wrappers_use():
    from sph3d_gcn_amd import tf_norm
    assert tf_norm.MAX_ROWS == N.MAX_ROWS == 2 ** 31 - 1024
