"""``consolver_amd.generate --type``: the reference's own flag (gen_ppo.py:402) beside ``--solver``, and ``make_type_scheduler``."""
import os

import pytest

import consolver_amd
from consolver_amd import generate as gen

SCHEDULES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "amed_schedules.json")


def test_types():
    assert gen.TYPES == ("consistencysolver", "unipc", "deis", "ipndm", "multistep-dpmsolver", "amed")
    assert gen.SOLVERS == ("consistencysolver", "multistep-dpmsolver", "ddim", "unipc", "amed")          # --solver is as it was


def test_parser():
    a = gen.parse_args(["--out", "o"])
    assert a.type is None and a.solver == "consistencysolver"
    for t in ("deis", "ipndm"):
        a = gen.parse_args(["--out", "o", "--type", t])
        assert a.type == t
    for t in ("consistencysolver", "unipc", "multistep-dpmsolver"):                # a type that is also a --solver value means the same
        a = gen.parse_args(["--out", "o", "--type", t])
        assert a.type == t and a.solver == t
        a = gen.parse_args(["--out", "o", "--type", t, "--solver", t])
        assert a.type == t and a.solver == t
    a = gen.parse_args(["--out", "o", "--type", "amed", "--amed-schedule", "f.json"])
    assert a.solver == "amed" and a.amed_schedule == "f.json"
    a = gen.parse_args(["--out", "o", "--type", "consistencysolver", "--policy", "p.ckpt", "--use_conv"])
    assert a.policy == "p.ckpt" and a.use_conv
    for bad in (["--type", "deis", "--solver", "unipc"], ["--type", "ipndm", "--solver", "consistencysolver"], ["--type", "unipc", "--solver=amed"],
                ["--type", "ddim"], ["--type", "dmdv2"], ["--solver", "deis"], ["--solver", "ipndm"],
                ["--type", "deis", "--policy", "p.ckpt"], ["--type", "ipndm", "--use_conv"], ["--type", "unipc", "--policy", "p.ckpt"],
                ["--type", "amed"], ["--type", "deis", "--amed-schedule", "f.json"]):
        with pytest.raises(SystemExit):
            gen.parse_args(["--out", "o"] + bad)


def test_make_type_scheduler():
    d = gen.make_type_scheduler("deis")
    assert type(d) is consolver_amd.DEISMultistepScheduler and d.factor_net is None and d.history_slots == 2
    c = d.config
    assert (c.beta_start, c.beta_end, c.beta_schedule, c.steps_offset) == (0.00085, 0.012, "scaled_linear", 1)
    assert (c.solver_order, c.algorithm_type, c.solver_type, c.lower_order_final, c.prediction_type, c.timestep_spacing) == \
        (2, "deis", "logrho", True, "epsilon", "linspace")
    p = gen.make_type_scheduler("ipndm")
    assert type(p) is consolver_amd.PNDMScheduler and p.factor_net is None and p.history_slots == 5
    c = p.config
    assert (c.beta_start, c.beta_end, c.beta_schedule, c.steps_offset) == (0.00085, 0.012, "scaled_linear", 1)
    assert (c.skip_prk_steps, c.set_alpha_to_one, c.prediction_type, c.timestep_spacing) == (True, False, "epsilon", "leading")
    assert consolver_amd.SD15_DEIS_KWARGS == dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1)
    assert consolver_amd.SD15_PNDM_KWARGS == dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True,
                                                  set_alpha_to_one=False, steps_offset=1)
    assert type(gen.make_type_scheduler("unipc")) is consolver_amd.UniPCMultistepScheduler
    assert type(gen.make_type_scheduler("multistep-dpmsolver")) is consolver_amd.DPMSolverMultistepScheduler
    s = gen.make_type_scheduler("consistencysolver", order_dim=3)
    assert type(s) is consolver_amd.PPOScheduler and s.config.order_dim == 3
    assert type(gen.make_type_scheduler("amed", amed_schedule=SCHEDULES)) is consolver_amd.AMEDSolverScheduler
    with pytest.raises(ValueError):
        gen.make_type_scheduler("amed")
    for bad in ("ddim", "dmdv2"):
        with pytest.raises(ValueError):
            gen.make_type_scheduler(bad)


def test_solver_flag_still_refuses_the_two_types():
    for t in ("deis", "ipndm"):
        with pytest.raises(ValueError):
            gen.make_scheduler(t)
        with pytest.raises(SystemExit):
            gen.parse_args(["--out", "o", "--solver", t])


def test_round_trip_through_the_config():
    for s in (gen.make_type_scheduler("deis"), gen.make_type_scheduler("ipndm")):
        t = type(s).from_config(s.config)
        assert type(t) is type(s) and {k: v for k, v in t.config.items() if not k.startswith("_")} == {k: v for k, v in s.config.items() if not k.startswith("_")}
