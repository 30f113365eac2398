!> Fortran host program driving lk_cg through ISO_C_BINDING only (no LightKrylov needed): conjugate gradient on the diagonal
!> SPD system d_i = 1 + (i-1)/n, b_i = sin(i), n = 1000, x0 = 0, at rtol = 1e-12 and the reference's atol.  Prints info, nres, the
!> tolerance, the last residual, max|b| and max|d x - b| so tests/test_gpu_cg_fortran.py can check them.
program test_cg_iso_c
    use, intrinsic :: iso_c_binding
    use lightkrylov_hip_c
    implicit none
    integer, parameter :: n = 1000, maxiter = 100
    type(c_ptr) :: ctx, Bb, Bx, W, A
    real(c_double), target :: d(n), b(n), x(n)
    real(c_double) :: res(maxiter + 1), rtol, atol, bnorm
    integer(c_int64_t) :: nres
    integer(c_int) :: rc, info
    integer :: i

    rc = lk_init(0_c_int, c_null_ptr, ctx); call chk(rc, 'lk_init')
    do i = 1, n
        d(i) = 1.0d0 + real(i - 1, c_double)/real(n, c_double)
        b(i) = sin(real(i, c_double))
    end do
    x = 0.0d0
    atol = 10.0d0**(-precision(1.0d0))          ! atol_dp, Constants.f90:35
    rtol = 1.0d-12
    rc = lk_basis_create(ctx, LK_F64, int(n, c_int64_t), 1_c_int, Bb); call chk(rc, 'lk_basis_create(b)')
    rc = lk_basis_create(ctx, LK_F64, int(n, c_int64_t), 1_c_int, Bx); call chk(rc, 'lk_basis_create(x)')
    rc = lk_basis_create(ctx, LK_F64, int(n, c_int64_t), 3_c_int, W); call chk(rc, 'lk_basis_create(W)')
    rc = lk_basis_upload(Bb, 0_c_int, 1_c_int, c_loc(b), int(n, c_int64_t)); call chk(rc, 'lk_basis_upload(b)')
    rc = lk_basis_upload(Bx, 0_c_int, 1_c_int, c_loc(x), int(n, c_int64_t)); call chk(rc, 'lk_basis_upload(x)')
    rc = lk_linop_diag_create(ctx, LK_F64, int(n, c_int64_t), c_loc(d), A); call chk(rc, 'lk_linop_diag_create')
    res = 0.0d0
    rc = lk_cg(A, c_null_ptr, Bb, 0_c_int, Bx, 0_c_int, W, rtol, atol, int(maxiter, c_int), res, int(size(res), c_int64_t), nres, info)
    call chk(rc, 'lk_cg')
    rc = lk_basis_download(Bx, 0_c_int, 1_c_int, c_loc(x), int(n, c_int64_t)); call chk(rc, 'lk_basis_download(x)')
    rc = lk_vec_norm(Bb, 0_c_int, bnorm); call chk(rc, 'lk_vec_norm(b)')
    print '(A,I0)', 'info ', info
    print '(A,I0)', 'nres ', nres
    print '(A,ES24.16)', 'tol ', atol + rtol*bnorm
    print '(A,ES24.16)', 'res_first ', res(1)
    print '(A,ES24.16)', 'res_last ', res(min(int(nres), size(res)))
    print '(A,ES24.16)', 'bmax ', maxval(abs(b))
    print '(A,ES24.16)', 'err ', maxval(abs(d*x - b))
    rc = lk_linop_destroy(A)
    rc = lk_basis_destroy(W)
    rc = lk_basis_destroy(Bx)
    rc = lk_basis_destroy(Bb)
    rc = lk_finalize(ctx)

contains
    subroutine chk(rc, what)
        integer(c_int), intent(in) :: rc
        character(len=*), intent(in) :: what
        if (rc /= LK_OK) then
            print '(A,A,A,I0,A,A)', 'ERROR in ', what, ': rc=', rc, ' ', lk_error_message()
            stop 1
        end if
    end subroutine
end program test_cg_iso_c
