"""GPU: the frame the six fused scheduler steps share (csrc/elementwise.hip step_fused_body / launch_step_fused) -- a launch with
`ticket` and `table` against the launches it replaces, bit for bit, for every entry point."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_STEPS = 3
# (latents [B, h, w, C], floats per table row): the smallest shapes at which the frame can go wrong
SHAPES = {
    "vec4_two_workgroups": ((2, 43, 3, 4), 8),        # B n = 1032: VEC = 4, 258 threads, the second workgroup nearly empty
    "vec1_odd_total": ((1, 23, 15, 3), 8),            # B n = 1035: VEC = 1, five workgroups
    "row_sets_the_grid": ((2, 43, 3, 4), 4096),       # 1024 threads for the row: two of the four workgroups hold no latent element
}


def _scheduler(solver):
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler
    if solver == "ddim":
        return DDIMScheduler()
    if solver == "dpm":
        return DPMSolverMultistepScheduler()
    return EulerAncestralDiscreteScheduler.from_config(DDIMScheduler().config)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("solver", ["ddim", "dpm", "euler_a"])
def test_step_with_ticket_and_table_equals_the_launches_it_replaces(solver, masked, shape):
    """Over 2 n_steps + 1 launches (the counter wraps twice), under CFG.  Unmasked: the fused launch against three launches -- the
    same solver's ticketless, tableless launch (DDIM: cfg_ddim_step), then advance_step and gather_row of the row it moved to; the
    Euler-ancestral draw ordinal also goes up by 1.  Masked, with a mask of ones: against the unmasked fused launch.  Compared bit for
    bit after every launch: x, x_in (both CFG halves), rowbias, the counter, t_out and hist / the Philox state; the ticket rests at 0."""
    from audioldm_with_lora_amd import ops
    dims, row = SHAPES[shape]
    B = dims[0]
    s = _scheduler(solver)
    s.set_timesteps(N_STEPS)
    coef, ts, blend = s.coefficient_table().cuda(), s.timesteps.float().cuda(), s.blend_table(0).cuda()
    g = torch.Generator().manual_seed(7)
    table = torch.randn(N_STEPS, row, generator=g).cuda()
    x_start = torch.randn(dims, generator=g)
    inpaint = (torch.randn(dims, generator=g).cuda(), torch.randn(dims, generator=g).cuda(), torch.ones(dims[:3]).cuda(), blend)

    def state():
        st = dict(x=x_start.clone().cuda(), x_in=torch.zeros((2 * B,) + dims[1:], dtype=torch.bfloat16, device="cuda"),
                  idx=torch.zeros(1, dtype=torch.int32, device="cuda"), t=ts[:1].clone(), rowbias=torch.zeros(row, device="cuda"))
        if solver == "dpm":
            st["op"] = torch.zeros(dims, device="cuda")                         # hist
        if solver == "euler_a":
            st["op"] = ops.philox_state(2025, 0xFFFFFFFE)                       # the ordinal's low word carries within the run
        return st

    def fused(st, with_mask):
        fn = getattr(ops, f"{solver}_step_fused" + ("_masked" if with_mask else ""))
        operand = (st["op"],) if "op" in st else ()
        fn(eps, st["x"], True, 2.5, coef, st["idx"], st["x_in"], *operand, table, st["rowbias"], ts, st["t"], ticket,
           *(inpaint if with_mask else ()))

    def three_launches(st):
        if solver == "ddim":
            ops.cfg_ddim_step(eps, st["x"], True, 2.5, coef, st["idx"], st["x_in"])
        else:
            getattr(ops, f"{solver}_step_fused")(eps, st["x"], True, 2.5, coef, st["idx"], st["x_in"], st["op"])
        if solver == "euler_a":
            seed, draw = ops.philox_state_values(st["op"])
            ops.philox_set(st["op"], draw=draw + 1)
        ops.advance_step(st["idx"], ts, st["t"])
        ops.gather_row(table, st["idx"], st["rowbias"])

    got, want = state(), state()
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in range(2 * N_STEPS + 1):
        eps = torch.randn((2 * B,) + dims[1:], generator=g).cuda()
        fused(got, masked)
        if masked:
            fused(want, False)
        else:
            three_launches(want)
        for name in got:
            assert torch.equal(_bits(got[name]), _bits(want[name])), (k, name)
        assert int(got["idx"]) == (k + 1) % N_STEPS and int(ticket) == 0, k
