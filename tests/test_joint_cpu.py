"""Joint rollouts without a GPU: the keying rule (mmt_sample.modality_seed) and the role planner of generate's list
form (model.plan_joint, model.joint_setting): every accepted form and every refusal that needs no device."""
import pytest
import torch

import mmt_sample as MS
import model as mmt_model
from model import GENERATED, GIVEN, HELD, plan_joint

V = [57, 13, 24, 5]
B, N0, N = 4, 5, 6
SHAPES = [(B, N0)] * 4


def test_modality_seed_pins():
    assert MS.modality_seed(0, 0) == 0xe220a8397b1dcdaf
    assert MS.modality_seed(0, 1) == 0x6e789e6aa1b965f4
    assert MS.modality_seed(0xC0FFEE1234, 0) == 0xfb68b820c78b9a30
    assert MS.modality_seed(0xC0FFEE1234, 3) == 0x282996a2b14a5be7
    assert MS.modality_seed(2 ** 64 - 1, 7) == 0x405da438a39e8064


def test_modality_seed_is_one_splitmix64_step_and_separates_modalities():
    def splitmix(x):
        x = (x + 0x9E3779B97F4A7C15) % 2 ** 64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        return z ^ (z >> 31)

    for seed in (0, 1, 0xC0FFEE1234, 2 ** 64 - 1):
        for i in range(8):
            assert MS.modality_seed(seed, i) == splitmix((seed + i * 0x9E3779B97F4A7C15) % 2 ** 64)
        assert len({MS.modality_seed(seed, i) for i in range(8)}) == 8
    assert MS.modality_seed(2 ** 64 + 5, 2) == MS.modality_seed(5, 2)  # modulo 2^64


def test_int_form_is_left_alone():
    for g in (0, 3, 7, -1):  # range checks of the int form stay where they were
        assert plan_joint(g, None, V, SHAPES, N) is None
    assert plan_joint(2, None, V, [(4, 5), (4, 9), (4, 5), (4, 5)], N) is None  # unequal prompts: the int form's rule
    with pytest.raises(ValueError):
        plan_joint(0, {1: torch.zeros(B, N, dtype=torch.long)}, V, SHAPES, N)  # given needs the list form


def test_list_forms_and_roles():
    p = plan_joint([2, 0, 3], None, V, SHAPES, N)
    assert p.roles == [GENERATED, HELD, GENERATED, GENERATED] and p.generated == [0, 2, 3] and p.given == {}
    assert (p.B, p.n0, p.N) == (B, N0, N)
    assert plan_joint((1,), None, V, SHAPES, N).roles == [HELD, GENERATED, HELD, HELD]  # a list of one is a list
    assert plan_joint("all", None, V, SHAPES, N).roles == [GENERATED] * 4
    assert plan_joint(range(2), None, V, SHAPES, N).generated == [0, 1]
    g1 = torch.randint(0, V[1], (B, N))
    p = plan_joint([0, 2], {1: g1}, V, SHAPES, N)
    assert p.roles == [GENERATED, GIVEN, GENERATED, HELD] and p.given[1] is g1
    # with num_samples a given is [B, N] (shared by a prompt's samples) or [B * S, N]
    assert plan_joint([0], {1: g1}, V, SHAPES, N, num_samples=3).roles[1] == GIVEN
    assert plan_joint([0], {3: torch.zeros(B * 3, N, dtype=torch.long)}, V, SHAPES, N, num_samples=3).roles[3] == GIVEN
    assert plan_joint([0], {1: torch.zeros(B, 0, dtype=torch.long)}, V, SHAPES, 0).N == 0
    # the edge tokens of the range
    edge = torch.tensor([[0, V[3] - 1] * (N // 2)] * B)
    assert plan_joint([0], {3: edge}, V, SHAPES, N).roles[3] == GIVEN


@pytest.mark.parametrize("g", [[0, 0], [0, 4], [-1], [1.0], [True], ["0"], [], "some", None, 2.5, True])
def test_refused_modality_arguments(g):
    with pytest.raises(ValueError):
        plan_joint(g, None, V, SHAPES, N)


def test_refused_given():
    ok = torch.zeros(B, N, dtype=torch.long)
    bad = {
        "generated and given": ([0, 1], {1: ok}),
        "dtype int32": ([0], {1: ok.int()}),
        "dtype float": ([0], {1: ok.float()}),
        "not a tensor": ([0], {1: [[0] * N] * B}),
        "too short": ([0], {1: ok[:, :-1]}),
        "wrong rows": ([0], {1: ok[:-1]}),
        "one-dimensional": ([0], {1: ok[0]}),
        "modality out of range": ([0], {4: ok}),
        "modality not an int": ([0], {"1": ok}),
        "token too large": ([0], {1: torch.full((B, N), V[1], dtype=torch.long)}),
        "token negative": ([0], {3: torch.tensor([[0] * (N - 1) + [-1]] * B)}),
        "not a dict": ([0], [ok]),
    }
    for what, (g, given) in bad.items():
        with pytest.raises(ValueError):
            plan_joint(g, given, V, SHAPES, N)
            pytest.fail(what)
    with pytest.raises(ValueError):  # [B * S, N] needs num_samples
        plan_joint([0], {1: torch.zeros(B * 3, N, dtype=torch.long)}, V, SHAPES, N)
    with pytest.raises(ValueError):
        plan_joint([0], {1: torch.zeros(B * 2, N, dtype=torch.long)}, V, SHAPES, N, num_samples=3)


def test_refused_prompts():
    for shapes in ([(4, 5), (4, 9), (4, 5), (4, 5)],  # unequal lengths
                   [(4, 5), (3, 5), (4, 5), (4, 5)],  # unequal batches
                   [(4, 5)] * 3,  # one prompt missing
                   [(4, 5, 1)] * 4, [(4,)] * 4, [(4, 0)] * 4):
        with pytest.raises(ValueError):
            plan_joint([0, 1], None, V, shapes, N)
    with pytest.raises(ValueError):
        plan_joint([0, 1], None, V, SHAPES, -1)


def test_joint_setting():
    assert mmt_model.joint_setting(0.8, [0, 2], "temperature") == {0: 0.8, 2: 0.8}
    assert mmt_model.joint_setting(None, [1], "top_k") == {1: None}
    assert mmt_model.joint_setting({2: 5}, [0, 2], "top_k") == {0: None, 2: 5}
    with pytest.raises(ValueError):
        mmt_model.joint_setting({1: 5}, [0, 2], "top_k")  # modality 1 is not generated


def test_generate_refuses_before_touching_a_device():
    """The refusals of generate's list form run before anything else: a model is not even needed up to there."""
    class Stub:
        vocab_sizes = V
        generate = mmt_model.MultimodalTransformer.generate

    prompts = [torch.zeros(B, N0, dtype=torch.long) for _ in V]
    fn = lambda probs: probs.argmax(-1, keepdim=True)  # noqa: E731
    with pytest.raises(ValueError, match="sample_fn"):
        Stub().generate(prompts, max_new_tokens=N, modality_to_generate=[0, 1], sample_fn=fn)
    with pytest.raises(ValueError, match="one shape"):
        Stub().generate([p[:, :3 + i] for i, p in enumerate(prompts)], max_new_tokens=N, modality_to_generate="all")
    with pytest.raises(ValueError, match="list form"):
        Stub().generate(prompts, max_new_tokens=N, modality_to_generate=0, given={1: torch.zeros(B, N, dtype=torch.long)})
