"""CPU: the C ABI and the host side of FlatAdamW with several parameter groups (wsis_adamw_group_bytes,
wsis_adamw_step_groups, wsis_adamw_step_scaled_groups; wsis_optim.group_rows, trainable, segment_groups,
group_param_indices, split_decay_groups).  Everything here returns before a kernel would be launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import wsis_native as _n
import wsis_optim as optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"wsis_adamw_group_bytes": 0, "wsis_adamw_step_groups": 6, "wsis_adamw_step_scaled_groups": 9}
WSIS_ERR_ARG = -1


def _declared_args(name):
    text = open(os.path.join(ROOT, "include", "wsis_hip.h")).read()
    m = re.search(r"^int(?:32_t)? " + name + r"\(([^)]*)\);", text, re.M)
    assert m, f"{name} is not declared in include/wsis_hip.h"
    args = " ".join(m.group(1).split())
    return 0 if args == "void" else args.count(",") + 1


def test_symbols_declared_exported_and_bound_with_the_declared_argument_counts():
    raw = ctypes.CDLL(os.path.join(ROOT, "3d-wsis_amd", "libwsis_hip.so"))
    _, hip_names = _n.declared_symbols()
    lib = _n.hip()
    for name, n_args in ARGS.items():
        assert _declared_args(name) == n_args, name
        assert hasattr(raw, name), name
        assert name in hip_names, name
        assert len(getattr(lib, name).argtypes) == n_args and getattr(lib, name).restype is _n.I32, name
    # the grouped entry points take the group table and its row count where the one-group ones take five doubles
    assert _declared_args("wsis_adamw_step") == len(lib.wsis_adamw_step.argtypes) == ARGS["wsis_adamw_step_groups"] + 3
    assert len(lib.wsis_adamw_step_scaled.argtypes) == ARGS["wsis_adamw_step_scaled_groups"] + 3
    assert lib.wsis_adamw_group_bytes() == 40 and lib.wsis_adamw_segment_bytes() == 56


def test_header_names_the_group_index_and_what_the_entry_points_replace():
    text = open(os.path.join(ROOT, "include", "wsis_hip.h")).read()
    assert "float g_clamp; int32_t group;}" in " ".join(text.split())
    entry = text[text.index("several parameter groups"):text.index("int32_t wsis_adamw_group_bytes(void);")]
    assert "train_scannetv2.py:93-94,251" in entry and "torch.optim.AdamW" in entry


def test_grouped_entry_points_check_their_arguments():
    lib = _n.hip()
    seg, blk, grp, skp = (ctypes.c_int64 * 7)(), (ctypes.c_int32 * 2)(), (ctypes.c_double * 5)(), (ctypes.c_int32 * 1)()
    a, b, g, c = (ctypes.addressof(x) for x in (seg, blk, grp, skp))
    plain = lambda *args: lib.wsis_adamw_step_groups(*args, None)                                   # noqa: E731
    scaled = lambda *args: lib.wsis_adamw_step_scaled_groups(*args[:5], None, None, args[5], None)  # noqa: E731
    assert plain(None, None, 0, g, 1) == 0 and scaled(None, None, 0, g, 1, None) == 0     # an empty step
    for call, rest in ((plain, ()), (scaled, (c,))):
        assert call(a, b, 1, g, 0, *rest) == WSIS_ERR_ARG
        assert call(a, b, 0, g, 0, *rest) == WSIS_ERR_ARG             # no group at all, even for an empty step
        assert call(a, b, 1, None, 1, *rest) == WSIS_ERR_ARG
        assert call(None, b, 1, g, 1, *rest) == WSIS_ERR_ARG
        assert call(a, None, 1, g, 1, *rest) == WSIS_ERR_ARG
        assert call(a, b, -1, g, 1, *rest) == WSIS_ERR_ARG
        assert call(a, b, 1 << 31, g, 1, *rest) == WSIS_ERR_ARG
    assert scaled(a, b, 1, g, 1, None) == WSIS_ERR_ARG
    assert b"wsis_adamw_step_scaled_groups" in lib.wsis_last_error()


def test_group_rows_hold_the_live_hyper_parameters_as_doubles():
    groups = [{"params": [], "lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-2, "initial_lr": 1.0},
              {"params": [], "lr": 0.0, "betas": [0.8, 0.99], "eps": 1e-6, "weight_decay": 0.0},
              {"params": [], "lr": np.float32(0.1), "betas": (torch.tensor(0.5).item(), 0.75), "eps": 1, "weight_decay": 5e-2}]
    rows = optim.group_rows(groups)
    assert rows.dtype == np.float64 and rows.shape == (3, 5) and rows.flags["C_CONTIGUOUS"]
    assert rows[0].tolist() == [1e-3, 0.9, 0.999, 1e-8, 1e-2]                  # lr, beta1, beta2, eps, weight_decay
    assert rows[1].tolist() == [0.0, 0.8, 0.99, 1e-6, 0.0]
    assert rows[2].tolist() == [float(np.float32(0.1)), 0.5, 0.75, 1.0, 5e-2]
    groups[0]["lr"] = 7e-4                                                     # a scheduler writes there
    assert optim.group_rows(groups)[0, 0] == 7e-4
    assert optim.group_rows(groups[:1]).shape == (1, 5)
    # 40 bytes a row, the layout of the kernel's struct; the segment table's int64 words carry them bit for bit
    words = rows.reshape(-1).view(np.int64)
    assert words.size == 15 and words.view(np.float64).tolist() == rows.reshape(-1).tolist()


def test_segment_to_group_mapping_after_the_requires_grad_filter():
    def t(n, grad=True):
        return torch.zeros(n, requires_grad=grad)
    lists = [[t(3), t(2, False), t(5)], [t(4, False), t(1, False)], [t(1)], [], [t(7), t(8), t(9, False)]]
    kept = [optim.trainable(g) for g in lists]
    assert [[p.numel() for p in g] for g in kept] == [[3, 5], [], [1], [], [7, 8]]
    assert kept[0][0] is lists[0][0] and kept[4][1] is lists[4][1]
    group_of = optim.segment_groups([len(g) for g in kept])
    assert group_of.dtype == np.int32 and group_of.tolist() == [0, 0, 2, 4, 4]   # the empty groups keep their indices
    assert optim.segment_groups([2]).tolist() == [0, 0]
    assert optim.segment_groups([0, 0, 1]).tolist() == [2]


def test_state_dict_indices_count_on_across_groups():
    assert optim.group_param_indices([2, 0, 1, 3]) == [[0, 1], [], [2], [3, 4, 5]]
    assert optim.group_param_indices([4]) == [[0, 1, 2, 3]]
    assert optim.group_param_indices([0, 2]) == [[], [0, 1]]
    # torch's own layout for the same groups
    p = [torch.zeros(1, requires_grad=True) for _ in range(6)]
    ref = torch.optim.AdamW([{"params": p[:2]}, {"params": p[2:3]}, {"params": p[3:]}])
    assert [g["params"] for g in ref.state_dict()["param_groups"]] == optim.group_param_indices([2, 1, 3])


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 3)
        self.bn = torch.nn.BatchNorm1d(3)
        self.frozen = torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.BatchNorm1d(3))
        self.head = torch.nn.Linear(3, 2, bias=False)
        self.tied = self.head                           # the same module twice: its weight is met once
        self.scale = torch.nn.Parameter(torch.ones(3))  # neither a bias nor a norm parameter
        for p in self.frozen.parameters():
            p.requires_grad_(False)


def test_split_decay_groups_covers_every_trainable_parameter_once():
    model = _Tiny()
    groups = optim.split_decay_groups(model, 1e-4)
    assert [g["weight_decay"] for g in groups] == [1e-4, 0.0] and all(set(g) == {"params", "weight_decay"} for g in groups)
    decay, plain = ([id(p) for p in g["params"]] for g in groups)
    assert decay == [id(model.scale), id(model.lin.weight), id(model.head.weight)]
    assert plain == [id(model.lin.bias), id(model.bn.weight), id(model.bn.bias)]
    trainable = [id(p) for p in model.parameters() if p.requires_grad]
    assert sorted(decay + plain) == sorted(trainable) and len(set(decay + plain)) == len(decay + plain)
    assert not {id(p) for p in model.frozen.parameters()} & set(decay + plain)
    # biases may keep their decay; other norm types may lose theirs
    groups = optim.split_decay_groups(model, 0.5, no_decay_bias=False)
    assert [id(p) for p in groups[1]["params"]] == [id(model.bn.weight), id(model.bn.bias)]
    assert id(model.lin.bias) in [id(p) for p in groups[0]["params"]] and groups[0]["weight_decay"] == 0.5
    groups = optim.split_decay_groups(model, 0.5, no_decay_types=(torch.nn.Linear,), no_decay_bias=False)
    assert [id(p) for p in groups[0]["params"]] == [id(model.scale), id(model.bn.weight), id(model.bn.bias)]
    # torch takes the pair as it is
    ref = torch.optim.AdamW(optim.split_decay_groups(model, 1e-4), lr=1e-3)
    assert [len(g["params"]) for g in ref.param_groups] == [3, 3]


def test_constructor_refusals_come_before_the_device():
    w = torch.zeros(3, requires_grad=True)
    for flag in ("amsgrad", "maximize", "foreach", "capturable"):
        with pytest.raises(ValueError, match=flag):
            optim.FlatAdamW([{"params": [w]}, {"params": [torch.zeros(2, requires_grad=True)], flag: True}])
    with pytest.raises(ValueError):
        optim.FlatAdamW([{"params": [torch.zeros(3)]}, {"params": []}])        # no parameter at all
    with pytest.raises(ValueError):
        optim.FlatAdamW([])
    with pytest.raises(ValueError):                                            # torch's rule: one group per parameter
        optim.FlatAdamW([{"params": [w]}, {"params": [w]}])
    with pytest.raises(_n.WsisError):                                          # several groups on the CPU: no fallback
        optim.FlatAdamW([{"params": [w], "lr": 1e-3}, {"params": [torch.zeros(2, requires_grad=True)], "lr": 1e-4}])
