"""Tools that study a host strategy itself -- the counterpart of ``hironaka/util`` (search.py)."""
from .search import (MorinTreeResult, SearchDepthResult, SearchTreeResult, TreeNodeData, search_depth, search_depths,
                     search_tree, search_tree_morin, search_trees, search_trees_morin)

__all__ = ["MorinTreeResult", "SearchDepthResult", "SearchTreeResult", "TreeNodeData", "search_depth", "search_depths",
           "search_tree", "search_tree_morin", "search_trees", "search_trees_morin"]
