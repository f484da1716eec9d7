"""Yogi (Zaheer et al. 2018) as a torch optimizer, in the FedYogi form of Adaptive Federated
Optimization (Reddi et al. 2021, Algorithm 2): no bias correction.

This class is the rule text the fused server step (csrc/server.hip, OK_YOGI) is pinned to: the
kernels compute, per element and with a correctly rounded sqrt, exactly the ops of step() below.
It runs on any device, holds its state as torch's optimizers do (step, exp_avg, exp_avg_sq), and
can be passed to FL.agents.Central(model, optim).

FedAdagrad needs no class of its own: with beta1 = 0 and lr_decay = 0 it is torch.optim.Adagrad.
"""
from __future__ import annotations

import torch


class Yogi(torch.optim.Optimizer):
    """exp_avg_sq starts at initial_accumulator_value (the paper's v_0 = tau^2 style floor; 1e-6)
    and moves additively: v -= (1 - beta2) * sign(v - g^2) * g^2."""

    def __init__(self, params, lr=1e-2, betas=(0.9, 0.99), eps=1e-3,
                 initial_accumulator_value=1e-6, weight_decay=0):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= initial_accumulator_value:
            raise ValueError(f"Invalid initial_accumulator_value value: {initial_accumulator_value}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps,
                                      initial_accumulator_value=initial_accumulator_value,
                                      weight_decay=weight_decay))

    @staticmethod
    def _sqrt(x):
        """exp_avg_sq.sqrt(); a test substitutes a correctly rounded one."""
        return x.sqrt()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr, eps, weight_decay = group["lr"], group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError("Yogi does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.full_like(
                        p, group["initial_accumulator_value"],
                        memory_format=torch.preserve_format)
                exp_avg, exp_avg_sq = state["exp_avg"], state["exp_avg_sq"]
                state["step"] += 1
                if weight_decay != 0:
                    g = g.add(p, alpha=weight_decay)
                exp_avg.lerp_(g, 1 - beta1)
                g2 = g * g
                exp_avg_sq.addcmul_(torch.sign(exp_avg_sq - g2), g2, value=-(1 - beta2))
                p.addcdiv_(exp_avg, self._sqrt(exp_avg_sq).add_(eps), value=-lr)
        return loss
