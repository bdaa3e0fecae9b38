"""CPU: what RoundEngine decides before any device work."""
import pytest

from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine


def test_removed_defer_mode_is_loud(monkeypatch):
    """FLR_DEFER_DEAD=1 (the side-stream dead-tap fill) was removed: asking for
    it raises instead of silently running another mode, before anything is
    allocated — so on a machine without a GPU too."""
    monkeypatch.setenv("FLR_DEFER_DEAD", "1")
    with pytest.raises(ValueError, match=r"removed.*profiles/r6_dead/"):
        RoundEngine(TINY, RoundConfig(num_clients=8, num_attackers=1), device="cpu")
