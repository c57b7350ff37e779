"""numpy fp64 oracle of UniPC (bh1 / bh2, orders 1 and 2, x0 prediction), written as the plain step-by-step algorithm.

Test infrastructure: shares no code with consolver_amd/scheduling_unipc.py or the kernel, and does not use the folded
per-step scalars -- every step converts the model output, runs the corrector of the previous update (differences D1, the
R / b system and an explicit ``np.linalg.solve``), stores the corrected sample and runs the predictor (Zhao et al. 2023,
UniPC alg. 5-6 in the B(h) form, in the sigma parametrisation diffusers 0.26.3 uses).  The beta table comes from
oracle/solver_oracle.py, which tests/golden pins to the reference.
"""
import itertools

import numpy as np

from oracle import solver_oracle as so


def combos(n):
    """solver_type x prediction_type x solver_order x disable_corrector ([], [0], every step)"""
    for st, pt, order, dc in itertools.product(("bh1", "bh2"), ("epsilon", "v_prediction"), (1, 2), ("none", "first", "all")):
        yield dict(solver_type=st, prediction_type=pt, solver_order=order,
                   disable_corrector={"none": [], "first": [0], "all": list(range(n))}[dc])


def combo_id(c):
    dc = c["disable_corrector"]
    return "-".join([c["solver_type"], c["prediction_type"], str(c["solver_order"]), "dc" + ("none" if not dc else "0" if dc == [0] else "all")])


class UniPCOracle:
    def __init__(self, num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="linear", solver_order=2,
                 prediction_type="epsilon", solver_type="bh2", lower_order_final=True, disable_corrector=(), timestep_spacing="linspace",
                 steps_offset=0, final_sigmas_type="sigma_min"):
        assert solver_order in (1, 2) and solver_type in ("bh1", "bh2")
        self.T = num_train_timesteps
        self.ac = so.alphas_cumprod(so.make_betas(beta_schedule, beta_start, beta_end, num_train_timesteps)).astype(np.float64)
        self.solver_order, self.prediction_type, self.solver_type = solver_order, prediction_type, solver_type
        self.lower_order_final, self.disable_corrector = lower_order_final, list(disable_corrector)
        self.timestep_spacing, self.steps_offset, self.final_sigmas_type = timestep_spacing, steps_offset, final_sigmas_type

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
        self.this_order = None
        self.last_sample = None
        self.corrected = None

    @staticmethod
    def alpha_sigma(sigma):
        alpha_t = 1.0 / (sigma ** 2 + 1.0) ** 0.5
        return alpha_t, sigma * alpha_t

    def lam(self, k):
        alpha, sigma = self.alpha_sigma(self.sigmas[k])
        with np.errstate(divide="ignore"):
            return np.log(alpha) - np.log(sigma)

    def convert_model_output(self, model_output, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index])
        if self.prediction_type == "epsilon":
            return (sample - sigma_t * model_output) / alpha_t
        return alpha_t * sample - sigma_t * model_output

    def rb(self, rks, hh, order):
        """the Vandermonde system of UniPC's B(h) form: rows R_j = rks^(j-1), right sides b_j = h phi_{j+1}(h) j! / B(h)"""
        h_phi_1 = np.expm1(hh)
        B_h = hh if self.solver_type == "bh1" else np.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1.0
        factorial_i = 1.0
        R, b = [], []
        for i in range(1, order + 1):
            R.append(np.asarray(rks, np.float64) ** (i - 1))
            b.append(h_phi_k * factorial_i / B_h)
            factorial_i *= i + 1
            h_phi_k = h_phi_k / hh - 1.0 / factorial_i
        return np.stack(R), np.asarray(b), h_phi_1, B_h

    def predictor(self, sample, order):
        """multistep UniP from grid position step_index to step_index + 1; model_outputs[-1] is this step's"""
        s0, t = self.step_index, self.step_index + 1
        m0 = self.model_outputs[-1]
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[t])
        _, sigma_s0 = self.alpha_sigma(self.sigmas[s0])
        if sigma_t == 0.0:                                       # the limit h -> inf of the first-order update
            assert order == 1
            return m0
        h = self.lam(t) - self.lam(s0)
        rks, D1s = [], []
        for i in range(1, order):
            mi = self.model_outputs[-(i + 1)]
            rk = (self.lam(s0 - i) - self.lam(s0)) / h
            rks.append(rk)
            D1s.append((mi - m0) / rk)
        rks.append(1.0)
        R, b, h_phi_1, B_h = self.rb(rks, -h, order)
        x_t_ = sigma_t / sigma_s0 * sample - alpha_t * h_phi_1 * m0
        if D1s:
            rhos_p = np.array([0.5]) if order == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
            pred_res = sum(rho * D1 for rho, D1 in zip(rhos_p, D1s))
        else:
            pred_res = 0.0
        return x_t_ - alpha_t * B_h * pred_res

    def corrector(self, this_model_output, last_sample, order):
        """multistep UniC over the previous grid step, step_index - 1 -> step_index; model_outputs[-1] is still the previous step's"""
        s0, t = self.step_index - 1, self.step_index
        m0 = self.model_outputs[-1]
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[t])
        _, sigma_s0 = self.alpha_sigma(self.sigmas[s0])
        h = self.lam(t) - self.lam(s0)
        rks, D1s = [], []
        for i in range(1, order):
            mi = self.model_outputs[-(i + 1)]
            rk = (self.lam(s0 - i) - self.lam(s0)) / h
            rks.append(rk)
            D1s.append((mi - m0) / rk)
        rks.append(1.0)
        R, b, h_phi_1, B_h = self.rb(rks, -h, order)
        rhos_c = np.array([0.5]) if order == 1 else np.linalg.solve(R, b)
        x_t_ = sigma_t / sigma_s0 * last_sample - alpha_t * h_phi_1 * m0
        corr_res = sum(rho * D1 for rho, D1 in zip(rhos_c[:-1], D1s)) if D1s else 0.0
        D1_t = this_model_output - m0
        return x_t_ - alpha_t * B_h * (corr_res + rhos_c[-1] * D1_t)

    def step(self, model_output, sample, round_m=None):
        """one step; ``round_m``: optional rounding applied to the converted output (the 16-bit history entry of the kernel)."""
        sample = np.asarray(sample, np.float64)
        m = self.convert_model_output(np.asarray(model_output, np.float64), sample)
        if round_m is not None:
            m = np.asarray(round_m(m), np.float64)
        use_corrector = self.step_index > 0 and (self.step_index - 1) not in self.disable_corrector and self.last_sample is not None
        if use_corrector:
            sample = self.corrector(m, self.last_sample, self.this_order)
        self.model_outputs = self.model_outputs[1:] + [m]
        this_order = min(self.solver_order, self.n - self.step_index) if self.lower_order_final else self.solver_order
        self.this_order = min(this_order, self.lower_order_nums + 1)
        self.last_sample = sample
        self.corrected = sample
        prev = self.predictor(sample, self.this_order)
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
