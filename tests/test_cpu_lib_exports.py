"""An export the binding calls but the loaded library lacks (an older build given through MARLMAZE_LIB) raises
the "rebuild the library" MMError, not a bare AttributeError -- and stays invisible to hasattr(), which the
loader uses to skip optional prototypes."""
import pytest

from marlmaze import _lib


class _Old:  # a library with one export
    def mm_version(self):
        return 1


def test_missing_export_raises_the_rebuild_error():
    L = _lib._Lib(_Old())
    assert L.mm_version() == 1
    with pytest.raises(_lib.MMError, match="no export mm_gemm_x2p_ok: rebuild the library"):
        L.mm_gemm_x2p_ok
    assert not hasattr(L, "mm_gemm_x2p_ok")


def test_x2p_ok_does_not_fall_back_on_a_stale_library(monkeypatch):
    """x3.x2p_ok asks the library; one without the export is an error, never a silent fp32-storage run."""
    from marlmaze import x3

    monkeypatch.setattr(_lib, "lib", lambda: _lib._Lib(_Old()))
    with pytest.raises(_lib.MMError, match="rebuild the library"):
        x3.x2p_ok(1000, 264, 264)
