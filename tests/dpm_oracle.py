"""numpy fp64 oracle of the Multistep DPM-Solver (orders 1 and 2), written as the plain step-by-step algorithm.

Test infrastructure: shares no code with consolver_amd/scheduling_dpm.py or the kernel, and does not use the folded
per-step scalars -- every step converts the model output, forms D0 / D1 and evaluates the published update formula
(Lu et al. 2022, DPM-Solver eq. 3.7 / DPM-Solver++ alg. 2, in the sigma parametrisation diffusers 0.26.3 uses).
The beta table comes from oracle/solver_oracle.py, which tests/golden pins to the reference.
"""
import itertools

import numpy as np

from oracle import solver_oracle as so


def combos():
    """algorithm_type x solver_order x solver_type x prediction_type x final_sigmas_type without the refused pair (dpmsolver with a zero final sigma)"""
    for alg, order, st, pt, fs in itertools.product(("dpmsolver", "dpmsolver++"), (1, 2), ("midpoint", "heun"), ("epsilon", "v_prediction"),
                                                    ("zero", "sigma_min")):
        if alg == "dpmsolver" and fs == "zero":
            continue
        yield dict(algorithm_type=alg, solver_order=order, solver_type=st, prediction_type=pt, final_sigmas_type=fs)


COMBOS = list(combos())


def combo_id(c):
    return "-".join(str(v) for v in c.values())


class DPMSolverOracle:
    def __init__(self, num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="linear", solver_order=2,
                 prediction_type="epsilon", algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                 euler_at_final=False, final_sigmas_type="zero", timestep_spacing="linspace", steps_offset=0):
        assert solver_order in (1, 2) and algorithm_type in ("dpmsolver", "dpmsolver++") and solver_type in ("midpoint", "heun")
        assert not (algorithm_type == "dpmsolver" and final_sigmas_type == "zero")
        self.T = num_train_timesteps
        self.ac = so.alphas_cumprod(so.make_betas(beta_schedule, beta_start, beta_end, num_train_timesteps)).astype(np.float64)
        self.solver_order, self.prediction_type, self.algorithm_type, self.solver_type = solver_order, prediction_type, algorithm_type, solver_type
        self.lower_order_final, self.euler_at_final, self.final_sigmas_type = lower_order_final, euler_at_final, final_sigmas_type
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset

    def set_timesteps(self, n):
        T = self.T
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1]
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1] + self.steps_offset
        else:
            ts = np.round(np.arange(T, 0, -T / n)) - 1
        self.timesteps = ts.astype(np.int64)
        all_sigmas = ((1 - self.ac) / self.ac) ** 0.5
        sig = np.interp(self.timesteps, np.arange(T), all_sigmas)
        last = all_sigmas[0] if self.final_sigmas_type == "sigma_min" else 0.0
        self.sigmas = np.concatenate([sig, [last]]).astype(np.float32).astype(np.float64)
        self.n = n
        self.step_index = 0
        self.model_outputs = [None] * self.solver_order          # oldest first
        self.lower_order_nums = 0

    @staticmethod
    def alpha_sigma(sigma):
        alpha_t = 1.0 / (sigma ** 2 + 1.0) ** 0.5
        return alpha_t, sigma * alpha_t

    def convert_model_output(self, model_output, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index])
        if self.algorithm_type == "dpmsolver++":              # data prediction
            if self.prediction_type == "epsilon":
                return (sample - sigma_t * model_output) / alpha_t
            return alpha_t * sample - sigma_t * model_output
        if self.prediction_type == "epsilon":                 # noise prediction
            return model_output
        return alpha_t * model_output + sigma_t * sample

    def first_order_update(self, m, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index + 1])
        alpha_s, sigma_s = self.alpha_sigma(self.sigmas[self.step_index])
        with np.errstate(divide="ignore"):
            lambda_t = np.log(alpha_t) - np.log(sigma_t)
        lambda_s = np.log(alpha_s) - np.log(sigma_s)
        h = lambda_t - lambda_s
        if self.algorithm_type == "dpmsolver++":
            return (sigma_t / sigma_s) * sample - (alpha_t * (np.exp(-h) - 1.0)) * m
        return (alpha_t / alpha_s) * sample - (sigma_t * (np.exp(h) - 1.0)) * m

    def second_order_update(self, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index + 1])
        alpha_s0, sigma_s0 = self.alpha_sigma(self.sigmas[self.step_index])
        alpha_s1, sigma_s1 = self.alpha_sigma(self.sigmas[self.step_index - 1])
        lambda_t = np.log(alpha_t) - np.log(sigma_t)
        lambda_s0 = np.log(alpha_s0) - np.log(sigma_s0)
        lambda_s1 = np.log(alpha_s1) - np.log(sigma_s1)
        m0, m1 = self.model_outputs[-1], self.model_outputs[-2]
        h, h_0 = lambda_t - lambda_s0, lambda_s0 - lambda_s1
        with np.errstate(divide="ignore"):                    # (h = 0 when a grid ends ON sigma_min: r0 = inf, D1 = 0, the step is the identity)
            r0 = h_0 / h
        D0, D1 = m0, (1.0 / r0) * (m0 - m1)
        if self.algorithm_type == "dpmsolver++":
            if self.solver_type == "midpoint":
                return (sigma_t / sigma_s0) * sample - (alpha_t * (np.exp(-h) - 1.0)) * D0 - 0.5 * (alpha_t * (np.exp(-h) - 1.0)) * D1
            return (sigma_t / sigma_s0) * sample - (alpha_t * (np.exp(-h) - 1.0)) * D0 + (alpha_t * ((np.exp(-h) - 1.0) / h + 1.0)) * D1
        if self.solver_type == "midpoint":
            return (alpha_t / alpha_s0) * sample - (sigma_t * (np.exp(h) - 1.0)) * D0 - 0.5 * (sigma_t * (np.exp(h) - 1.0)) * D1
        return (alpha_t / alpha_s0) * sample - (sigma_t * (np.exp(h) - 1.0)) * D0 - (sigma_t * ((np.exp(h) - 1.0) / h - 1.0)) * D1

    def step(self, model_output, sample, round_m=None):
        """one step; ``round_m``: optional rounding applied to the converted output (the 16-bit history entry of the kernel)."""
        sample = np.asarray(sample, np.float64)
        m = self.convert_model_output(np.asarray(model_output, np.float64), sample)
        if round_m is not None:
            m = np.asarray(round_m(m), np.float64)
        self.model_outputs = self.model_outputs[1:] + [m]
        last = self.step_index == self.n - 1
        lower_final = last and (self.euler_at_final or (self.lower_order_final and self.n < 15) or self.final_sigmas_type == "zero")
        if self.solver_order == 1 or self.lower_order_nums < 1 or lower_final:
            prev = self.first_order_update(m, sample)
        else:
            prev = self.second_order_update(sample)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return prev

    def last_converted(self):
        return self.model_outputs[-1]


def run(oracle, eps_fn, x, n):
    """n-step trajectory with the model ``eps_fn(x, t)``; returns the list of samples after every step."""
    oracle.set_timesteps(n)
    xs = []
    x = np.asarray(x, np.float64)
    for t in oracle.timesteps:
        x = oracle.step(eps_fn(x, int(t)), x)
        xs.append(x)
    return xs
