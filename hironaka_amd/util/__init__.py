"""Tools that study a host strategy itself -- the counterpart of ``hironaka/util`` (search.py)."""
from .search import (SearchDepthResult, SearchTreeResult, TreeNodeData, search_depth, search_depths, search_tree,
                     search_trees)

__all__ = ["SearchDepthResult", "SearchTreeResult", "TreeNodeData", "search_depth", "search_depths", "search_tree",
           "search_trees"]
