"""Tools that study a host strategy itself -- the counterpart of ``hironaka/util`` (search.py)."""
from .search import SearchDepthResult, search_depth, search_depths

__all__ = ["SearchDepthResult", "search_depth", "search_depths"]
