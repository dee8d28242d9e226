// corbo-hip-stage: name=input_envelope slot=3 kind=state_control_ineq rows=4 nx_min=3 nu_min=2
//
// A USER stage inequality that couples a state with the controls, FOUR rows: a state-dependent envelope on the first two inputs,
//     e_i = prm[2 i] + prm[2 i + 1] * x[2] * x[2]        (i = 0, 1; every product and sum left to right)
//     c(x, u) = [u[0] - e_0,  -u[0] - e_0,  u[1] - e_1,  -u[1] - e_1] <= 0,          i.e. |u_i| <= a_i + b_i x[2]^2
// -- a torque-speed envelope, a speed-dependent steering limit (unicycle: x[2] is the heading; quadrotor: x[2] the altitude).  The NON-INTEGRAL
// STATE-CONTROL TERM (dimension 4) of a user's corbo::StageInequalityConstraint subclass: see drive_power.hpp for the edge and where it is created.
template <> struct StageFunction<3> {
    static constexpr int KIND = CORBO_HIP_STAGE_FN_STATE_CONTROL_INEQ;
    static constexpr int ROWS = 4;
    template <int NX, int NU>
    __host__ __device__ static __forceinline__ void value(const double* x, const double* u, const double* prm, double* out)
    {
        if constexpr (NX >= 3 && NU >= 2) {
            const double e0 = prm[0] + prm[1] * x[2] * x[2];
            const double e1 = prm[2] + prm[3] * x[2] * x[2];
            out[0] = u[0] - e0;
            out[1] = -u[0] - e0;
            out[2] = u[1] - e1;
            out[3] = -u[1] - e1;
        }
        else out[0] = out[1] = out[2] = out[3] = 0.0;
    }
};
