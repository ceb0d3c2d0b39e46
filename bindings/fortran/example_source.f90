!> The device run of example_gaussian.f90 with the likelihood written as device source: the text is compiled at run time for the
!! GPU the run is on and evaluated inside the sampling kernel, like the built-in Gaussian.
program example_source
    use iso_c_binding
    use polychord_hip
    implicit none
    integer, parameter :: nDims = 4, nDerived = 1
    character(len=*), parameter :: nl = new_line('a')
    ! likelihoods/examples/gaussian.f90: N(mu, sigma^2 I) with (mu, sigma) = the data block, phi_1 = radius
    character(len=*), parameter :: source = &
        "__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived," // nl // &
        "                                      const double *data, long ndata)" // nl // &
        "{" // nl // &
        "    double r2 = 0.0;" // nl // &
        "    for (int i = 0; i < nDims; ++i) r2 += (theta[i] - data[0]) * (theta[i] - data[0]);" // nl // &
        "    if (nDerived > 0) phi[0] = sqrt(r2);" // nl // &
        "    return -nDims * (log(data[1]) + 0.5 * log(6.283185307179586)) - 0.5 * r2 / (data[1] * data[1]);" // nl // &
        "}" // nl // c_null_char
    real(c_double) :: block(2)
    integer(c_int) :: handle
    block = [0.5d0, 0.1d0]
    handle = pchip_source_create(source, c_null_char, block, 2_c_long)
    if (handle <= 0) stop 2
    if (polychord_hip_set_source(handle) /= 0) stop 2
    call run_polychord_hip(c_funloc(polychord_hip_source_loglike), c_funloc(polychord_hip_uniform_prior), nDims, nDerived, 200, 8, &
                           "chains", "f_source", 3, .false., .true., .true.)
    if (polychord_hip_set_source(0_c_int) /= 0) stop 2
    call pchip_source_destroy(handle)
end program example_source
