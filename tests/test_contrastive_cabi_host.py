"""ia_contrastive_fwd / ia_contrastive_bwd refuse bad arguments before any launch: the codes come back on a machine with no GPU, as
tests/test_cabi_symbols.py::test_error_codes_without_touching_the_gpu has it for the older entry points.  The pointers are addresses of
host buffers that no call here gets far enough to touch."""
import ctypes

import pytest

ERR_ARG, ERR_WS = -1, -3
B, H = 4, 16


@pytest.fixture(scope="module")
def lib():
    from item_alignment_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    b = ctypes.create_string_buffer(4096)
    return ctypes.addressof(b), b


def test_workspace_size(lib):
    assert lib.ia_contrastive_workspace_bytes(0) == 0 and lib.ia_contrastive_workspace_bytes(-2) == 0
    for b in (1, 2, 64, 65, 257):
        n = lib.ia_contrastive_workspace_bytes(b)
        assert n >= (b * b + b) * 4 and n >= 2 * b * 4 and n % 256 == 0


def test_forward_refuses_before_any_launch(lib, buf):
    p, _keep = buf
    ws = lib.ia_contrastive_workspace_bytes(B)

    def fwd(t=p, ldt=H, im=p, ldi=H, ls=p, sim=p, lds=B, lr=p, lc=p, lo=p, b=B, h=H, w=p, wb=ws):
        return lib.ia_contrastive_fwd(t, ldt, im, ldi, ls, sim, lds, lr, lc, lo, b, h, w, wb, None)

    for kw in (dict(t=None), dict(im=None), dict(ls=None), dict(sim=None), dict(lr=None), dict(lc=None), dict(lo=None), dict(b=0),
               dict(b=-1), dict(h=0), dict(h=-5), dict(ldt=H - 1), dict(ldi=H - 1), dict(lds=B - 1), dict(ldt=0), dict(lds=0)):
        assert fwd(**kw) == ERR_ARG, kw
    for kw in (dict(w=None), dict(wb=ws - 1), dict(wb=0)):
        assert fwd(**kw) == ERR_WS, kw


def test_backward_refuses_before_any_launch(lib, buf):
    p, _keep = buf
    ws = lib.ia_contrastive_workspace_bytes(B)

    def bwd(t=p, ldt=H, im=p, ldi=H, ls=p, sim=p, lds=B, lr=p, lc=p, dl=p, dt=p, lddt=H, di=p, lddi=H, dls=p, acc=0, b=B, h=H, w=p, wb=ws):
        return lib.ia_contrastive_bwd(t, ldt, im, ldi, ls, sim, lds, lr, lc, dl, dt, lddt, di, lddi, dls, acc, b, h, w, wb, None)

    for kw in (dict(t=None), dict(im=None), dict(ls=None), dict(sim=None), dict(lr=None), dict(lc=None), dict(dl=None), dict(dt=None),
               dict(di=None), dict(dls=None), dict(b=0), dict(b=-1), dict(h=0), dict(h=-5), dict(ldt=H - 1), dict(ldi=H - 1),
               dict(lds=B - 1), dict(lddt=H - 1), dict(lddi=H - 1)):
        assert bwd(**kw) == ERR_ARG, kw
    for kw in (dict(w=None), dict(wb=ws - 1), dict(wb=0)):
        assert bwd(**kw) == ERR_WS, kw


def test_codes_are_the_header_s(lib):
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "itemalign.h")).read()
    assert int(re.search(r"#define IA_ERR_ARG \((-?\d+)\)", header).group(1)) == ERR_ARG
    assert int(re.search(r"#define IA_ERR_WORKSPACE \((-?\d+)\)", header).group(1)) == ERR_WS
    assert lib.ia_strerror(ERR_WS).decode() != lib.ia_strerror(ERR_ARG).decode()
