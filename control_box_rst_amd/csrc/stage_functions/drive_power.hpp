// corbo-hip-stage: name=drive_power slot=2 kind=state_control_ineq rows=1 nx_min=3 nu_min=1
//
// A USER stage inequality that couples a STATE with a CONTROL, dropped into csrc/stage_functions/: a drive-power bound |u[0] x[2]| <= P, written smooth,
//     c(x, u) = (u[0] * x[2])^2 - prm[0]^2 <= 0          (the cart-pole's force times x[2], a velocity-like state; prm[0] = the power limit P)
// -- the NON-INTEGRAL STATE-CONTROL TERM (here of dimension 1) of a user's corbo::StageInequalityConstraint subclass (getNonIntegralStateControlTermDimension /
// computeNonIntegralStateControlTerm: one BinaryVectorVertexEdge on (x_k, u_k) per interval behind the control term's edge and in front of the
// control-deviation edge, nlp_functions.cpp:109-115).  Public id CORBO_HIP_STAGE_FN_USER + slot in corbo_hip_problem_desc::stage_ineq_state_control, parameters
// through corbo_hip_set_state_control_params.  An edge inside the stage block (x_k, u_k): the sweep kernel's extra-edge instantiation evaluates it, the
// block-tridiagonal / band routes factorise.  `value` writes ROWS values; the vertex dimensions are template parameters like the kernels instantiate them.
template <> struct StageFunction<2> {
    static constexpr int KIND = CORBO_HIP_STAGE_FN_STATE_CONTROL_INEQ;
    static constexpr int ROWS = 1;
    template <int NX, int NU>
    __host__ __device__ static __forceinline__ void value(const double* x, const double* u, const double* prm, double* out)
    {
        if constexpr (NX >= 3 && NU >= 1) {
            const double pw = u[0] * x[2];
            out[0] = pw * pw - prm[0] * prm[0];
        }
        else out[0] = 0.0;
    }
};
