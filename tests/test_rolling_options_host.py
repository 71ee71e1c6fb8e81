"""SelfPlay's `rolling` / `search_options` validation as a pure function (mcts.rolling_options): the accepted forms, every
refusal, the default quantum with and without a playout cap, and the producer handing the option to its children.  No GPU."""
import pytest

from hive_alphazero_amd import mcts

CAP = {"full": 50, "fast": 10, "p_full": 0.25}


def test_accepted_forms_of_rolling():
    opt = mcts.rolling_options
    for off in (None, False, 0, {}):
        assert opt(off, None, 8, 1) is None
    assert opt(None, {"keep_tree": True}, 8, 1) is None                      # lock step keeps trees
    assert opt(True, None, 8, 1) == {"quantum": 8}
    assert opt(True, {"share_equal_leaves": False, "keep_tree": False}, 8, 3) == {"quantum": 4}
    assert opt({"quantum": 3}, None, 8, 1) == {"quantum": 3}
    given = {"quantum": 2}
    assert opt(given, {}, 8, 2) == given and opt(given, {}, 8, 2) is not given


def test_default_quantum_with_and_without_a_cap():
    opt = mcts.rolling_options
    # without a cap: the rounds of the one search length, 1 + ceil((sims - 1) / slots)
    assert opt(True, None, 50, 1)["quantum"] == 50 == mcts.rolling_quantum(50, 1)
    assert opt(True, None, 50, 4)["quantum"] == 14 == mcts.rolling_quantum(50, 4)
    # with a cap: the rounds of the SHORTER search, whichever of full / fast that is
    assert opt(True, None, 50, 1, CAP)["quantum"] == 10
    assert opt(True, None, 50, 4, CAP)["quantum"] == 4 == mcts.rolling_quantum(10, 4)
    assert opt(True, None, 50, 1, {"full": 10, "fast": 50, "p_full": 0.5})["quantum"] == 10
    assert opt({"quantum": 7}, None, 50, 1, CAP)["quantum"] == 7            # a given quantum stands
    assert opt({"quantum": 0}, None, 8, 1)["quantum"] == 8                  # 0 = not given


def test_every_refusal():
    opt = mcts.rolling_options
    for bad in ({"rounds": 2}, {"quantum": 2, "keep_tree": True}, {"quantum": -1}):
        with pytest.raises(ValueError):
            opt(bad, None, 8, 1)
    for rolling in (True, {"quantum": 2}):
        with pytest.raises(ValueError, match="keep trees"):
            opt(rolling, {"keep_tree": True}, 8, 1)


def test_producer_hands_the_dict_to_its_children_unchanged():
    from hive_alphazero_amd import self_play
    rolling = {"quantum": 3}
    w = self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], row_format="compact", playout_cap=CAP, rolling=rolling)
    assert w.cfg["rolling"] == rolling and w.cfg["rolling"] is not rolling
    # what the child does with it: mcts.SelfPlay(rolling=cfg["rolling"]) parses it to the same option
    assert mcts.rolling_options(w.cfg["rolling"], None, 50, 1, w.cfg["playout_cap"]) == {"quantum": 3}
