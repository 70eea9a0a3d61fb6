"""ctypes mirror of ``include/hironaka_hip.h`` (constants, descriptors, prototypes).

Kept free of torch so the CPU-side tests (and the oracle binding, which takes the same
descriptors with host pointers) can import it without a GPU.
"""
import ctypes as C

HK_ABI_VERSION = 6

# status codes
HK_OK = 0
HK_ERR_NULL = -1
HK_ERR_SHAPE = -2
HK_ERR_UNSUPPORTED = -3
HK_ERR_ALIGN = -4
HK_ERR_LAUNCH = -5
HK_ERR_NO_DEVICE = -6

# scalar dtypes
HK_F32, HK_F64, HK_I32, HK_I64, HK_U8 = 0, 1, 2, 3, 4

# coordinate-subset kinds (a mask's dtype code, or one of these)
HK_COORDS_CLASS_I32 = 16
HK_COORDS_CLASS_I64 = 17
HK_COORDS_IN_RECORD = 18
HK_AXIS_MASKED_LOGITS = 32
HK_COORDS_NONE = 19

# stages
HK_STAGE_SHIFT = 1
HK_STAGE_REPOSITION = 2
HK_STAGE_NEWTON = 4
HK_STAGE_RESCALE = 8

# semantics + behaviour flags
HK_SEM_JAX, HK_SEM_TORCH, HK_SEM_LIST, HK_SEM_MASK = 0, 1, 2, 3
HK_FLAG_AXIS_NOOP_IF_INVALID = 4
HK_FLAG_IGNORE_ENDED = 8
HK_FLAG_COMPACT_SORTED = 16
HK_FLAG_FORCE_GENERIC = 32
HK_FLAG_FORCE_TEAM = 64
HK_FLAG_DEFER_COUNTS = 128
HK_FLAG_FORCE_ONE_LANE = 256
HK_FLAG_FORCE_TWO_LANES = 512
HK_FLAG_FORCE_FOUR_LANES = 1024

# fused policies
HK_HOST_RANDOM, HK_HOST_ALL_COORD, HK_HOST_ZEILLINGER = 0, 1, 2
HK_HOST_ZEILLINGER_LEX, HK_HOST_WEAK_SPIVAKOVSKY, HK_HOST_MIN_HITTING = 3, 4, 5  # hk_host_select / hk_search_depth
HK_HOST_SPIVAKOVSKY, HK_HOST_RANDOM_SPIVAKOVSKY = 6, 7  # hk_spivakovsky_select only (hironaka_hip_spivakovsky.h)
HK_AGENT_RANDOM, HK_AGENT_RANDOM_LEGAL, HK_AGENT_CHOOSE_FIRST, HK_AGENT_CHOOSE_LAST = 0, 1, 2, 3

# hk_search_depth / hk_search_game_tree status bits
HK_SEARCH_DEPTH_LIMIT = 1
HK_SEARCH_NODE_LIMIT = 2
HK_SEARCH_STACK_LIMIT = 4
HK_SEARCH_INEXACT = 8
HK_SEARCH_ROOT_ENDED = 16
HK_SEARCH_ROOT_INVALID = 32  # hk_search_morin_tree

# hk_search_morin_play: outcomes, tie modes, weight rules, flag, the "every class is forced" host code
HK_MORIN_RUNNING, HK_MORIN_ENDED, HK_MORIN_NO_CONTRIBUTION, HK_MORIN_NO_MOVE, HK_MORIN_INEXACT = 0, 1, 2, 3, 4
HK_MORIN_TIE_LOWEST, HK_MORIN_TIE_HIGHEST, HK_MORIN_TIE_RANDOM = 0, 1, 2
HK_MORIN_WEIGHTS_AGENT, HK_MORIN_WEIGHTS_SEARCH = 0, 1
HK_MORIN_REDUCE_ROOT = 1
HK_MORIN_HOST_FORCED = -1

# hk_game_play: outcomes (the numbers of the HK_MORIN_* codes they share), flags, the "every class is forced" host code
HK_PLAY_RUNNING, HK_PLAY_ENDED, HK_PLAY_NO_MOVE, HK_PLAY_INEXACT, HK_PLAY_VALUE_LIMIT = 0, 1, 3, 4, 5
HK_PLAY_REPOSITION, HK_PLAY_RESCALE, HK_PLAY_REDUCE_ROOT, HK_PLAY_RESCALE_ROOT = 1, 2, 4, 8
HK_PLAY_HOST_FORCED = -1

# hk_env_step: modes, descriptor flags
HK_ENV_MODE_HOST, HK_ENV_MODE_AGENT = 0, 1
HK_ENV_SCALE_OBSERVATION, HK_ENV_STOP_AFTER_INVALID, HK_ENV_STOP_AT_THRESHOLD, HK_ENV_POINT_REDUCTION_REWARD = 1, 2, 4, 8
HK_ENV_IMPROVE_EFFICIENCY, HK_ENV_AGENT_REPOSITION, HK_ENV_AUTO_RESET, HK_ENV_RESET_ALL = 16, 32, 64, 128

# hk_dqn_agent_move: descriptor flags
HK_DQN_MOVE_MASKED, HK_DQN_MOVE_RESCALE = 1, 2

# hk_tree_expand: descriptor flags, the bit of its status word
HK_TREE_REPOSITION, HK_TREE_ZERO_TAIL = 1, 2
HK_TREE_OVERFLOW = 1

# hk_replay_push / hk_replay_sample: the cursor's words, the Philox stream of the sample indices, rows per workgroup
HK_REPLAY_MAX_COLS, HK_REPLAY_CURSOR_WORDS = 8, 8
HK_REPLAY_POS, HK_REPLAY_FULL, HK_REPLAY_LAST_COUNT, HK_REPLAY_TOTAL_PUSHED = 0, 1, 2, 3
HK_REPLAY_SAMPLES_DRAWN, HK_REPLAY_TICKET = 4, 5
HK_REPLAY_STREAM = 4
HK_REPLAY_TILE_ROWS = 128

# hk_dqn_td / hk_polyak_update: rows per workgroup, the action limit, the bit of the status word; tensors per launch,
# the bytes of one tensor a workgroup owns
HK_DQN_TILE_ROWS, HK_DQN_MAX_ACTIONS, HK_DQN_BAD_ACTION = 256, 65536, 1
HK_POLYAK_MAX_TENSORS, HK_POLYAK_CHUNK_BYTES = 64, 16384

# hk_optim_prepare / hk_optim_apply: tensors per launch, the bytes of one gradient a workgroup owns, the bytes of the
# state block; kinds; flags
HK_OPTIM_MAX_TENSORS, HK_OPTIM_CHUNK_BYTES, HK_OPTIM_STATE_BYTES = 64, 16384, 64
HK_OPTIM_SCALE, HK_OPTIM_SGD, HK_OPTIM_ADAM = 0, 1, 2
HK_OPTIM_LAST, HK_OPTIM_ADVANCE, HK_OPTIM_KEEP_GRADS, HK_OPTIM_NESTEROV, HK_OPTIM_NO_CLIP = 1, 2, 4, 8, 16

# hk_mlp_forward: the table's length, the widest layer, the row tiles and the largest batch on the small one; descriptor
# flags; the layer flag
HK_MLP_MAX_LAYERS, HK_MLP_MAX_WIDTH = 32, 256
HK_MLP_TILE_SMALL, HK_MLP_TILE_LARGE, HK_MLP_TILE_CROSSOVER = 16, 64, 4096
HK_MLP_INPUT_RELU, HK_MLP_FORCE_TILE_SMALL, HK_MLP_FORCE_TILE_LARGE = 1, 2, 4
HK_MLP_RELU = 1
# hk_train_mlp_forward / hk_train_mlp_backward: the largest batch, the rows of the small instantiation, the layer flag
HK_MLP_TRAIN_MAX_BATCH, HK_MLP_TRAIN_ROWS_SMALL = 1024, 256
HK_MLP_TRAIN_BN = 2
# hk_pvnet_forward: the table's length, the widest layer, the block kinds and the descriptor flags (the FORCE bits are
# hk_mlp_forward's)
HK_PVNET_MAX_BLOCKS, HK_PVNET_MAX_WIDTH = 32, 256
HK_PVNET_DENSE, HK_PVNET_RESIDUE = 0, 1
HK_PVNET_RAW_VALUE, HK_PVNET_FORCE_TILE_SMALL, HK_PVNET_FORCE_TILE_LARGE = 1, 2, 4
# hk_pv_loss: rows per workgroup, the action limit (the policy head's), the bit of the status word
HK_PVLOSS_TILE_ROWS, HK_PVLOSS_MAX_ACTIONS, HK_PVLOSS_BAD_INDEX = 16, 255, 1
# hk_pvgrad_forward / hk_pvgrad_backward: the largest batch (the 16-row tile's range), Denses per parameter-gradient launch
HK_PVGRAD_MAX_BATCH, HK_PVGRAD_TABLE = 4096, 40
# hk_customnet_forward: the most points, and the descriptor flags (hk_pvnet_forward's)
HK_CUSTOMNET_MAX_POINTS = 64
HK_CUSTOMNET_RAW_VALUE, HK_CUSTOMNET_FORCE_TILE_SMALL, HK_CUSTOMNET_FORCE_TILE_LARGE = 1, 2, 4
PVNET_NORMED_WIDTHS = (32, 64, 128, 256)  # the widths of a normed layer the kernel serves (1, 2, 4, 8 columns per group)

SEMANTICS = {"jax": HK_SEM_JAX, "torch": HK_SEM_TORCH, "list": HK_SEM_LIST}


class hk_step_desc(C.Structure):
    _fields_ = [
        ("points_in", C.c_void_p),
        ("points_out", C.c_void_p),
        ("in_stride", C.c_int64),
        ("out_stride", C.c_int64),
        ("coords", C.c_void_p),
        ("coords_stride", C.c_int64),
        ("axis", C.c_void_p),
        ("done_out", C.c_void_p),
        ("prev_done_out", C.c_void_p),
        ("reward_out", C.c_void_p),
        ("num_points_out", C.c_void_p),
        ("padding_value", C.c_double),
        ("reward_sign", C.c_float),
        ("batch", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("coords_kind", C.c_int32),
        ("axis_dtype", C.c_int32),
        ("stages", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class hk_rollout_desc(C.Structure):
    _fields_ = [
        ("points", C.c_void_p),
        ("points_in", C.c_void_p),
        ("done_count", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("obs_out", C.c_void_p),
        ("host_class_out", C.c_void_p),
        ("axis_out", C.c_void_p),
        ("done_out", C.c_void_p),
        ("reward_out", C.c_void_p),
        ("game_length_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("game_offset", C.c_uint64),
        ("step_offset", C.c_uint32),
        ("padding_value", C.c_double),
        ("reward_sign", C.c_float),
        ("batch", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("steps", C.c_int32),
        ("host_policy", C.c_int32),
        ("agent_policy", C.c_int32),
        ("stages", C.c_uint32),
        ("flags", C.c_uint32),
        ("game_ids", C.c_void_p),
        ("gen_max_value", C.c_int32),
        ("gen_stages", C.c_uint32),
        ("gen_seed", C.c_uint64),
        ("episodes", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class hk_search_tree(C.Structure):
    _fields_ = [
        ("node_visits", C.c_void_p),
        ("raw_values", C.c_void_p),
        ("node_values", C.c_void_p),
        ("parents", C.c_void_p),
        ("action_from_parent", C.c_void_p),
        ("children_index", C.c_void_p),
        ("children_prior_logits", C.c_void_p),
        ("children_visits", C.c_void_p),
        ("children_rewards", C.c_void_p),
        ("children_discounts", C.c_void_p),
        ("children_values", C.c_void_p),
        ("batch", C.c_int32),
        ("num_nodes", C.c_int32),
        ("num_actions", C.c_int32),
    ]


class hk_morin_play_desc(C.Structure):
    _fields_ = [
        ("points_in", C.c_void_p),
        ("points_out", C.c_void_p),
        ("in_stride", C.c_int64),
        ("out_stride", C.c_int64),
        ("weights_in", C.c_void_p),
        ("weights_out", C.c_void_p),
        ("distinguished_in", C.c_void_p),
        ("distinguished_out", C.c_void_p),
        ("class_in", C.c_void_p),
        ("axis_in", C.c_void_p),
        ("class_out", C.c_void_p),
        ("axis_out", C.c_void_p),
        ("length_out", C.c_void_p),
        ("outcome_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("game_offset", C.c_uint64),
        ("batch", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("host", C.c_int32),
        ("max_steps", C.c_int32),
        ("tie", C.c_int32),
        ("weight_rule", C.c_int32),
        ("flags", C.c_uint32),
        ("step_offset", C.c_uint32),
    ]


class hk_game_play_desc(C.Structure):
    _fields_ = [
        ("points_in", C.c_void_p),
        ("points_out", C.c_void_p),
        ("in_stride", C.c_int64),
        ("out_stride", C.c_int64),
        ("class_in", C.c_void_p),
        ("axis_in", C.c_void_p),
        ("class_out", C.c_void_p),
        ("axis_out", C.c_void_p),
        ("length_out", C.c_void_p),
        ("outcome_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("game_offset", C.c_uint64),
        ("value_threshold", C.c_double),
        ("batch", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("host", C.c_int32),
        ("agent", C.c_int32),
        ("max_steps", C.c_int32),
        ("flags", C.c_uint32),
        ("step_offset", C.c_uint32),
        ("reserved_", C.c_uint32),
    ]


class hk_env_step_desc(C.Structure):
    _fields_ = [
        ("points_in", C.c_void_p),
        ("points_out", C.c_void_p),
        ("class_io", C.c_void_p),
        ("step_count", C.c_void_p),
        ("episode", C.c_void_p),
        ("action", C.c_void_p),
        ("reward", C.c_void_p),
        ("stopped", C.c_void_p),
        ("exceed", C.c_void_p),
        ("obs_points", C.c_void_p),
        ("obs_coords", C.c_void_p),
        ("final_points", C.c_void_p),
        ("final_coords", C.c_void_p),
        ("agent_axis", C.c_void_p),
        ("seed", C.c_uint64),
        ("agent_seed", C.c_uint64),
        ("game_offset", C.c_uint64),
        ("world_games", C.c_uint64),
        ("value_threshold", C.c_double),
        ("invalid_move_penalty", C.c_double),
        ("threshold_penalty", C.c_double),
        ("batch", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("mode", C.c_int32),
        ("host", C.c_int32),
        ("agent", C.c_int32),
        ("max_value", C.c_int32),
        ("step_threshold", C.c_int32),
        ("flags", C.c_uint32),
    ]


class hk_dqn_host_move_desc(C.Structure):
    _fields_ = [
        ("q", C.c_void_p),
        ("q_stride", C.c_int64),
        ("class_out", C.c_void_p),
        ("coords_out", C.c_void_p),
        ("prev_done", C.c_void_p),
        ("counts", C.c_void_p),
        ("batch", C.c_int32),
        ("dim", C.c_int32),
        ("q_dtype", C.c_int32),
        ("coords_dtype", C.c_int32),
    ]


class hk_dqn_agent_move_desc(C.Structure):
    _fields_ = [
        ("points", C.c_void_p),
        ("q", C.c_void_p),
        ("q_stride", C.c_int64),
        ("class_id", C.c_void_p),
        ("axis_out", C.c_void_p),
        ("features_out", C.c_void_p),
        ("done_out", C.c_void_p),
        ("lengths", C.c_void_p),
        ("counts", C.c_void_p),
        ("padding_value", C.c_double),
        ("batch", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("q_dtype", C.c_int32),
        ("flags", C.c_uint32),
    ]


class hk_tree_expand_desc(C.Structure):
    _fields_ = [
        ("parents_in", C.c_void_p),
        ("children_out", C.c_void_p),
        ("in_stride", C.c_int64),
        ("out_stride", C.c_int64),
        ("class_id", C.c_void_p),
        ("child_offset", C.c_void_p),
        ("child_parent", C.c_void_p),
        ("child_axis", C.c_void_p),
        ("child_num_points", C.c_void_p),
        ("child_done", C.c_void_p),
        ("status", C.c_void_p),
        ("n_parents", C.c_int32),
        ("capacity", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("sem", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved_", C.c_uint32),
    ]


class hk_replay_col(C.Structure):
    _fields_ = [
        ("ring", C.c_void_p),
        ("rows", C.c_void_p),
        ("row_bytes", C.c_int64),
        ("rows_stride_bytes", C.c_int64),
    ]


class hk_replay_desc(C.Structure):
    _fields_ = [
        ("col", hk_replay_col * HK_REPLAY_MAX_COLS),
        ("keep", C.c_void_p),
        ("cursor", C.c_void_p),
        ("ncols", C.c_int32),
        ("batch", C.c_int32),
        ("capacity", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class hk_dqn_td_desc(C.Structure):
    _fields_ = [
        ("q", C.c_void_p),
        ("next_q", C.c_void_p),
        ("actions", C.c_void_p),
        ("rewards", C.c_void_p),
        ("dones", C.c_void_p),
        ("target", C.c_void_p),
        ("row_loss", C.c_void_p),
        ("dq", C.c_void_p),
        ("loss", C.c_void_p),
        ("workspace", C.c_void_p),
        ("status", C.c_void_p),
        ("q_stride", C.c_int64),
        ("next_q_stride", C.c_int64),
        ("dq_stride", C.c_int64),
        ("gamma", C.c_double),
        ("batch", C.c_int32),
        ("num_actions", C.c_int32),
        ("dtype", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class hk_pv_loss_desc(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p),
        ("value", C.c_void_p),
        ("target_policy", C.c_void_p),
        ("target_value", C.c_void_p),
        ("weight", C.c_void_p),
        ("index", C.c_void_p),
        ("dlogits", C.c_void_p),
        ("dvalue", C.c_void_p),
        ("row_loss", C.c_void_p),
        ("loss", C.c_void_p),
        ("workspace", C.c_void_p),
        ("status", C.c_void_p),
        ("logits_stride", C.c_int64),
        ("value_stride", C.c_int64),
        ("target_policy_stride", C.c_int64),
        ("dlogits_stride", C.c_int64),
        ("dvalue_stride", C.c_int64),
        ("num_samples", C.c_int64),
        ("batch", C.c_int32),
        ("actions", C.c_int32),
        ("dtype", C.c_int32),
        ("flags", C.c_int32),
    ]


class hk_polyak_tensor(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("numel", C.c_int64),
    ]


class hk_polyak_desc(C.Structure):
    _fields_ = [
        ("tensor", hk_polyak_tensor * HK_POLYAK_MAX_TENSORS),
        ("tau", C.c_double),
        ("ntensors", C.c_int32),
        ("dtype", C.c_int32),
    ]


class hk_optim_tensor(C.Structure):
    _fields_ = [
        ("param", C.c_void_p),
        ("grad", C.c_void_p),
        ("state1", C.c_void_p),
        ("state2", C.c_void_p),
        ("numel", C.c_int64),
    ]


class hk_optim_state(C.Structure):
    _fields_ = [
        ("step", C.c_int64),
        ("beta1_pow", C.c_double),
        ("beta2_pow", C.c_double),
        ("total_norm", C.c_double),
        ("clip_coef", C.c_double),
        ("neg_step_size", C.c_double),
        ("bias2_sqrt", C.c_double),
        ("lr", C.c_double),
    ]


class hk_optim_desc(C.Structure):
    _fields_ = [
        ("tensor", hk_optim_tensor * HK_OPTIM_MAX_TENSORS),
        ("state", C.c_void_p),
        ("workspace", C.c_void_p),
        ("lr_dev", C.c_void_p),
        ("lr", C.c_double),
        ("beta1", C.c_double),
        ("beta2", C.c_double),
        ("eps", C.c_double),
        ("weight_decay", C.c_double),
        ("momentum", C.c_double),
        ("dampening", C.c_double),
        ("max_norm", C.c_double),
        ("ntensors", C.c_int32),
        ("dtype", C.c_int32),
        ("kind", C.c_int32),
        ("slot_base", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved_", C.c_int32),
    ]


class hk_mlp_layer(C.Structure):
    _fields_ = [
        ("weight", C.c_void_p),
        ("bias", C.c_void_p),
        ("bn_mean", C.c_void_p),
        ("bn_var", C.c_void_p),
        ("bn_weight", C.c_void_p),
        ("bn_bias", C.c_void_p),
        ("eps", C.c_float),
        ("k", C.c_int32),
        ("n", C.c_int32),
        ("flags", C.c_uint32),
    ]


class hk_mlp_desc(C.Structure):
    _fields_ = [
        ("x0", C.c_void_p),
        ("x1", C.c_void_p),
        ("out", C.c_void_p),
        ("in_bn_mean", C.c_void_p),
        ("in_bn_var", C.c_void_p),
        ("in_bn_weight", C.c_void_p),
        ("in_bn_bias", C.c_void_p),
        ("x0_stride", C.c_int64),
        ("x1_stride", C.c_int64),
        ("out_stride", C.c_int64),
        ("batch", C.c_int32),
        ("k0", C.c_int32),
        ("k1", C.c_int32),
        ("nlayers", C.c_int32),
        ("dtype", C.c_int32),
        ("flags", C.c_uint32),
        ("in_eps", C.c_float),
        ("reserved_", C.c_int32),
        ("layer", hk_mlp_layer * HK_MLP_MAX_LAYERS),
    ]


class hk_mlp_train_layer(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in (
        "weight", "bias", "bn_weight", "bn_bias", "running_mean", "running_var", "num_batches_tracked", "z", "act",
        "mean", "inv", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias")] + [
        ("eps", C.c_float),
        ("momentum", C.c_float),
        ("k", C.c_int32),
        ("n", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved_", C.c_int32),
    ]


class hk_mlp_train_desc(C.Structure):
    _fields_ = [
        ("x0", C.c_void_p),
        ("x1", C.c_void_p),
        ("grad_out", C.c_void_p),
        ("workspace", C.c_void_p),
        ("x0_stride", C.c_int64),
        ("x1_stride", C.c_int64),
        ("grad_stride", C.c_int64),
        ("workspace_bytes", C.c_uint64),
        ("batch", C.c_int32),
        ("k0", C.c_int32),
        ("k1", C.c_int32),
        ("nlayers", C.c_int32),
        ("dtype", C.c_int32),
        ("flags", C.c_uint32),
        ("layer", hk_mlp_train_layer * HK_MLP_MAX_LAYERS),
    ]


class hk_pvnet_dense(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("weight", "bias", "gn_scale", "gn_bias")]


class hk_pvnet_block(C.Structure):
    _fields_ = [
        ("dense1", hk_pvnet_dense),
        ("dense2", hk_pvnet_dense),
        ("proj", hk_pvnet_dense),
        ("eps", C.c_float),
        ("k", C.c_int32),
        ("n", C.c_int32),
        ("kind", C.c_int32),
    ]


class hk_pvnet_desc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p),
        ("policy", C.c_void_p),
        ("value", C.c_void_p),
        ("policy_weight", C.c_void_p),
        ("policy_bias", C.c_void_p),
        ("value_weight", C.c_void_p),
        ("value_bias", C.c_void_p),
        ("x_stride", C.c_int64),
        ("policy_stride", C.c_int64),
        ("value_stride", C.c_int64),
        ("batch", C.c_int32),
        ("k0", C.c_int32),
        ("nblocks", C.c_int32),
        ("actions", C.c_int32),
        ("dtype", C.c_int32),
        ("flags", C.c_uint32),
        ("block", hk_pvnet_block * HK_PVNET_MAX_BLOCKS),
    ]


class hk_customnet_desc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p),
        ("policy", C.c_void_p),
        ("value", C.c_void_p),
        ("towers", C.c_void_p),
        ("policy_weight", C.c_void_p),
        ("policy_bias", C.c_void_p),
        ("value_weight", C.c_void_p),
        ("value_bias", C.c_void_p),
        ("workspace", C.c_void_p),
        ("gate", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("x_stride", C.c_int64),
        ("policy_stride", C.c_int64),
        ("value_stride", C.c_int64),
        ("batch", C.c_int32),
        ("m", C.c_int32),
        ("d", C.c_int32),
        ("e", C.c_int32),
        ("nblocks", C.c_int32),
        ("n_last", C.c_int32),
        ("actions", C.c_int32),
        ("want", C.c_int32),
        ("dtype", C.c_int32),
        ("flags", C.c_uint32),
    ]


class hk_pvgrad_dense(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("d_weight", "d_bias", "d_gn_scale", "d_gn_bias")]


class hk_pvgrad_block(C.Structure):
    _fields_ = [("dense1", hk_pvgrad_dense), ("dense2", hk_pvgrad_dense), ("proj", hk_pvgrad_dense)]


class hk_pvgrad_desc(C.Structure):
    _fields_ = [
        ("net", hk_pvnet_desc),
        ("grad_policy", C.c_void_p),
        ("grad_value", C.c_void_p),
        ("workspace", C.c_void_p),
        ("grad_policy_stride", C.c_int64),
        ("grad_value_stride", C.c_int64),
        ("workspace_bytes", C.c_uint64),
        ("policy", hk_pvgrad_dense),
        ("value", hk_pvgrad_dense),
        ("block", hk_pvgrad_block * HK_PVNET_MAX_BLOCKS),
    ]


# include/hironaka_hip_customgrad.h: offsets in floats into one gradient buffer; NONE: not there
HK_CUSTOMGRAD_NONE = -1
HK_CUSTOMGRAD_HEADER, HK_CUSTOMGRAD_FIRST, HK_CUSTOMGRAD_SIZE = 144, 4, 72


class hk_customgrad_dense(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ("d_weight", "d_bias", "d_gn_scale", "d_gn_bias")]


class hk_customgrad_block(C.Structure):
    _fields_ = [("dense1", hk_customgrad_dense), ("dense2", hk_customgrad_dense), ("proj", hk_customgrad_dense)]


class hk_customgrad_desc(C.Structure):
    _fields_ = [
        ("net", hk_customnet_desc),
        ("grad_table", C.c_void_p),
        ("grads", C.c_void_p),
        ("grad_policy", C.c_void_p),
        ("grad_value", C.c_void_p),
        ("grad_policy_stride", C.c_int64),
        ("grad_value_stride", C.c_int64),
        ("grad_floats", C.c_uint64),
        ("policy", hk_customgrad_dense),
        ("value", hk_customgrad_dense),
        ("n", C.c_int32 * HK_PVNET_MAX_BLOCKS),
        ("kind", C.c_int32 * HK_PVNET_MAX_BLOCKS),
    ]


# include/hironaka_hip_unified.h
HK_UNIFIED_REPOSITION, HK_UNIFIED_SCALE_OBSERVATION = 1, 2
HK_UNIFIED_MAX_DIM = 5  # the search takes at most 32 actions


class hk_unified_expand_desc(C.Structure):
    _fields_ = [
        ("embeddings", C.c_void_p),
        ("parent", C.c_void_p),
        ("action", C.c_void_p),
        ("node", C.c_void_p),
        ("kind", C.c_void_p),
        ("net_in", C.c_void_p),
        ("subset", C.c_void_p),
        ("reward", C.c_void_p),
        ("discount_out", C.c_void_p),
        ("discount", C.c_float),
        ("batch", C.c_int32),
        ("num_nodes", C.c_int32),
        ("max_points", C.c_int32),
        ("dim", C.c_int32),
        ("dtype", C.c_int32),
        ("flags", C.c_uint32),
    ]


_vp, _i, _i64, _u32, _u64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_double

# name -> (restype, argtypes) of every symbol the header declares.  `stream` is the trailing
# void* of the device entry points; the oracle exports the same list with prefix hko_ and
# without the stream argument.
PROTOTYPES = {
    "hk_abi_version": (C.c_int, []),
    "hk_strerror": (C.c_char_p, [_i]),
    "hk_has_fast_path": (C.c_int, [_i, _i, _i]),
    "hk_step": (C.c_int, [C.POINTER(hk_step_desc), _vp]),
    "hk_shift": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _d, _u32, _vp]),
    "hk_reposition": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _d, _u32, _vp]),
    "hk_get_newton_polytope": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _d, _u32, _vp]),
    "hk_rescale": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _d, _u32, _vp]),
    "hk_get_dones": (C.c_int, [_vp, _i64, _vp, _i, _i, _i, _i, _vp]),
    "hk_get_num_points": (C.c_int, [_vp, _i64, _vp, _i, _i, _i, _i, _vp]),
    "hk_generate_points": (C.c_int, [_vp, _i, _i, _i, _i, _i, _u64, _u64, _u32, _d, _u32, _vp]),
    "hk_bin_group_games": (C.c_int, [_i, _i, _i]),
    "hk_bin_unit_games": (C.c_int, [_i, _i, _i]),
    "hk_generate_points_binned": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _u64, _u64, _u32, _d, _u32, _vp]),
    "hk_bin_by_live_rows": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "hk_rollout": (C.c_int, [C.POINTER(hk_rollout_desc), _vp]),
    "hk_rollout_workspace_bytes": (C.c_uint64, [C.POINTER(hk_rollout_desc)]),
    "hk_rollout_reduce_counts": (C.c_int, [C.POINTER(hk_rollout_desc), C.c_void_p]),
    "hk_search_select": (C.c_int, [C.POINTER(hk_search_tree), _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "hk_search_backup": (C.c_int, [C.POINTER(hk_search_tree), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hk_search_policy": (C.c_int, [C.POINTER(hk_search_tree), _vp, _vp, _vp, _vp, _vp]),
    "hk_zeillinger": (C.c_int, [_vp, _i64, _vp, _i, _i, _i, _i, _u32, _vp]),
    "hk_get_features": (C.c_int, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _d, _vp]),
    "hk_get_features_torch": (C.c_int, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _d, _vp]),
    "hk_decode_host_class": (C.c_int, [_vp, _vp, _i, _i, _i, _vp]),
    "hk_step_features": (C.c_int, [C.POINTER(hk_step_desc), _vp, _i, _vp]),
    "hk_rollout_values": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, C.c_float, C.c_float, C.c_float, _vp]),
    "hk_search_expand_gather": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "hk_search_masked_argmax": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp]),
    "hk_search_expand_scatter": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "hk_search_expand_gather_agent": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "hk_search_expand_scatter_agent": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "hk_search_mask_logits": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp]),
    "hk_search_depth_workspace_bytes": (C.c_uint64, [_i, _i, _i, _i, _i]),
    "hk_search_depth": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _u64, _i, _vp, _u64, _vp, _vp, _vp, _vp]),
    "hk_search_game_tree_workspace_bytes": (C.c_uint64, [_i, _i, _i, _i, _i, _i]),
    "hk_search_game_tree": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i64, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp]),
    "hk_search_morin_tree_workspace_bytes": (C.c_uint64, [_i, _i, _i, _i, _i, _i]),
    "hk_search_morin_tree": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i64, _i, _i, _i, _vp, _u64, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hk_search_morin_play": (C.c_int, [C.POINTER(hk_morin_play_desc), _vp]),
}

STATUS_TEXT = {
    HK_OK: "ok",
    HK_ERR_NULL: "a required pointer is NULL",
    HK_ERR_SHAPE: "batch / max_points / dim / stride / class id out of range",
    HK_ERR_UNSUPPORTED: "dtype, kind or flag combination not supported",
    HK_ERR_ALIGN: "pointer not aligned to its element size",
    HK_ERR_LAUNCH: "HIP kernel launch failed",
    HK_ERR_NO_DEVICE: "no HIP device",
}


# the entry points of include/hironaka_hip_hosts.h: the device library's only (no hko_ counterpart in the oracle)
DEVICE_PROTOTYPES = {
    "hk_host_select": (C.c_int, [_vp, _i64, _vp, _i, _i, _i, _i, _i, _vp]),
}

# the entry point of include/hironaka_hip_play.h: the device library's only, as above
PLAY_PROTOTYPES = {
    "hk_game_play": (C.c_int, [C.POINTER(hk_game_play_desc), _vp]),
}

# the entry point of include/hironaka_hip_tree.h: the device library's only, as above
TREE_PROTOTYPES = {
    "hk_tree_expand": (C.c_int, [C.POINTER(hk_tree_expand_desc), _vp]),
}

# the entry point of include/hironaka_hip_env.h: the device library's only, as above
ENV_PROTOTYPES = {
    "hk_env_step": (C.c_int, [C.POINTER(hk_env_step_desc), _vp]),
}

# the entry points of include/hironaka_hip_replay.h: the device library's only, as above
REPLAY_PROTOTYPES = {
    "hk_replay_push": (C.c_int, [C.POINTER(hk_replay_desc), _vp]),
    "hk_replay_sample": (C.c_int, [C.POINTER(hk_replay_desc), _i, _u64, _vp, _vp]),
}

# the entry points of include/hironaka_hip_dqn.h: the device library's only, as above
DQN_PROTOTYPES = {
    "hk_dqn_td_workspace_bytes": (C.c_uint64, [_i]),
    "hk_dqn_td": (C.c_int, [C.POINTER(hk_dqn_td_desc), _vp]),
    "hk_polyak_update": (C.c_int, [C.POINTER(hk_polyak_desc), _vp]),
}

# the entry points of include/hironaka_hip_optim.h: the device library's only, as above
OPTIM_PROTOTYPES = {
    "hk_optim_workspace_bytes": (C.c_uint64, [_i64]),
    "hk_optim_prepare": (C.c_int, [C.POINTER(hk_optim_desc), _vp]),
    "hk_optim_apply": (C.c_int, [C.POINTER(hk_optim_desc), _vp]),
}

# the entry points of include/hironaka_hip_mlp.h: the device library's only, as above
MLP_PROTOTYPES = {
    "hk_mlp_row_tile": (C.c_int, [_i64]),
    "hk_mlp_forward": (C.c_int, [C.POINTER(hk_mlp_desc), _vp]),
}

# the entry points of include/hironaka_hip_mlp_train.h: the device library's only, as above
MLP_TRAIN_PROTOTYPES = {
    "hk_train_mlp_rows": (C.c_int, [_i64]),
    "hk_train_mlp_workspace_bytes": (C.c_uint64, [C.POINTER(hk_mlp_train_desc)]),
    "hk_train_mlp_forward": (C.c_int, [C.POINTER(hk_mlp_train_desc), _vp]),
    "hk_train_mlp_backward": (C.c_int, [C.POINTER(hk_mlp_train_desc), _vp]),
}

# the entry point of include/hironaka_hip_pvnet.h: the device library's only, as above
PVNET_PROTOTYPES = {
    "hk_pvnet_forward": (C.c_int, [C.POINTER(hk_pvnet_desc), _vp]),
}

# the entry points of include/hironaka_hip_customnet.h: the device library's only, as above
CUSTOMNET_PROTOTYPES = {
    "hk_customnet_workspace_bytes": (C.c_uint64, [_i64, C.c_int32]),
    "hk_customnet_forward": (C.c_int, [C.POINTER(hk_customnet_desc), _vp]),
}

# the entry points of include/hironaka_hip_pvloss.h: the device library's only, as above
PVLOSS_PROTOTYPES = {
    "hk_pv_loss_workspace_bytes": (C.c_uint64, [_i]),
    "hk_pv_loss": (C.c_int, [C.POINTER(hk_pv_loss_desc), _vp]),
}

# the entry points of include/hironaka_hip_pvgrad.h: the device library's only, as above
PVGRAD_PROTOTYPES = {
    "hk_pvgrad_workspace_bytes": (C.c_uint64, [C.POINTER(hk_pvgrad_desc)]),
    "hk_pvgrad_forward": (C.c_int, [C.POINTER(hk_pvgrad_desc), _vp]),
    "hk_pvgrad_backward": (C.c_int, [C.POINTER(hk_pvgrad_desc), _vp]),
}

# the entry points of include/hironaka_hip_customgrad.h: the device library's only, as above
CUSTOMGRAD_PROTOTYPES = {
    "hk_customgrad_workspace_bytes": (C.c_uint64, [C.POINTER(hk_customgrad_desc)]),
    "hk_customgrad_forward": (C.c_int, [C.POINTER(hk_customgrad_desc), _vp]),
    "hk_customgrad_backward": (C.c_int, [C.POINTER(hk_customgrad_desc), _vp]),
}

# the entry points of include/hironaka_hip_unified.h: the device library's only, as above
UNIFIED_PROTOTYPES = {
    "hk_unified_expand": (C.c_int, [C.POINTER(hk_unified_expand_desc), _vp]),
    "hk_unified_prior": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "hk_unified_pvnet_forward": (C.c_int, [C.POINTER(hk_pvnet_desc), _vp, C.c_int32, _vp]),
}

# the entry point of include/hironaka_hip_spivakovsky.h: the device library's only, as above
SPIVAKOVSKY_PROTOTYPES = {
    "hk_spivakovsky_select": (C.c_int, [_vp, _i64, _vp, _i, _i, _i, _i, _i, _u64, _u64, _u32, _vp]),
}

# the entry points of include/hironaka_hip_dqn_move.h: the device library's only, as above
DQN_MOVE_PROTOTYPES = {
    "hk_dqn_host_move": (C.c_int, [C.POINTER(hk_dqn_host_move_desc), _vp]),
    "hk_dqn_agent_move": (C.c_int, [C.POINTER(hk_dqn_agent_move_desc), _vp]),
}


def bind(lib: C.CDLL, prototypes=None) -> None:
    """Attach restype/argtypes (default: PROTOTYPES, DEVICE_PROTOTYPES, PLAY_PROTOTYPES, TREE_PROTOTYPES, ENV_PROTOTYPES,
    REPLAY_PROTOTYPES, DQN_PROTOTYPES, OPTIM_PROTOTYPES, MLP_PROTOTYPES, MLP_TRAIN_PROTOTYPES, PVNET_PROTOTYPES,
    CUSTOMNET_PROTOTYPES, PVLOSS_PROTOTYPES, PVGRAD_PROTOTYPES, CUSTOMGRAD_PROTOTYPES, UNIFIED_PROTOTYPES, SPIVAKOVSKY_PROTOTYPES and DQN_MOVE_PROTOTYPES); raises
    AttributeError for a symbol the library lacks."""
    if prototypes is None:
        prototypes = {**PROTOTYPES, **DEVICE_PROTOTYPES, **PLAY_PROTOTYPES, **TREE_PROTOTYPES, **ENV_PROTOTYPES,
                      **REPLAY_PROTOTYPES, **DQN_PROTOTYPES, **OPTIM_PROTOTYPES, **MLP_PROTOTYPES,
                      **MLP_TRAIN_PROTOTYPES, **PVNET_PROTOTYPES, **CUSTOMNET_PROTOTYPES, **PVLOSS_PROTOTYPES,
                      **PVGRAD_PROTOTYPES, **CUSTOMGRAD_PROTOTYPES, **UNIFIED_PROTOTYPES, **SPIVAKOVSKY_PROTOTYPES,
                      **DQN_MOVE_PROTOTYPES}
    for name, (res, args) in prototypes.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
