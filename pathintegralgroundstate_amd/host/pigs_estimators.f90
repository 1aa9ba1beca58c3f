!-----------------------------------------------------------------------
! pigs_estimators -- host-side structural estimators, block statistics and the output
! files of the front end (formats of the reference: vpi.f90:517-518, sample_mod.f90:392-932).
! These are O(Nbin) / O(Np^2) once per step (<2 % of the reference's run time, SURVEY §3);
! the O(Np^2 * beads) energy sums are GPU kernels behind pigs_capi.
!-----------------------------------------------------------------------
module pigs_estimators

  implicit none
  private
  public :: est_params, pair_correlation, structure_factor, obdm_accumulate
  public :: normalize_gr, normalize_sk, normalize_nr, variance, perm_state, perm_sampling
  public :: write_radial, write_sk, write_nr
  public :: normalize_density, write_density, write_profile
  public :: normalize_fqt, write_fqt
  public :: normalize_sqv, sqv_shells, sqv_shell_means, write_sqvec, write_sqshell
  public :: normalize_fqv, write_fqvec, write_fqshell
  public :: normalize_msd, write_msd
  public :: normalize_grv, write_grvec
  public :: normalize_tau, write_tau
  public :: normalize_bop, write_bo, write_boh
  public :: normalize_vh, write_vh
  public :: normalize_g3, write_g3, write_g3ang
  public :: normalize_atm, atm_window_mean, v3_header, write_v3_block, write_v3tau
  public :: normalize_lat, lat_nn_distance, lind_header, write_lind_block, write_lindtau, write_usite
  public :: normalize_sf, sf_columns, write_rhos, write_msdu
  public :: normalize_cl, clus_header, write_clus_block, write_clus
  public :: normalize_pc, perc_header, write_perc_block, write_percsz, write_clpers
  public :: normalize_nk, normalize_nrvec, n0_header, write_n0_block, write_nkvec

  type est_params
     integer :: dim = 3, Np = 0, Nbin = 100, Nk = 50, Npw = 0
     logical :: trap = .false.
     real(8) :: rcut2 = 0.d0, rbin = 0.d0, pi = 0.d0, CWorm = 0.d0
     real(8) :: Lbox(3) = 1.d0, LboxHalf(3) = 0.5d0, qbin(3) = 0.d0
  end type est_params

  ! permutation-cycle bookkeeping of one walker (reference sample_mod.f90:530-594)
  type perm_state
     logical :: new_cycle = .false., end_cycle = .false.
     integer :: iperm = 1
     integer, allocatable :: members(:), histogram(:)
  end type perm_state

contains

  function image_r2(p,x) result(r2)
    type(est_params), intent(in) :: p
    real(8), intent(inout) :: x(p%dim)
    real(8) :: r2
    integer :: k
    r2 = 0.d0
    do k=1,p%dim
       if (x(k)> p%LboxHalf(k)) x(k) = x(k)-p%Lbox(k)
       if (x(k)<-p%LboxHalf(k)) x(k) = x(k)+p%Lbox(k)
       r2 = r2+x(k)*x(k)
    end do
  end function image_r2

  ! g(r) histogram of one slice: +2 per pair inside the cutoff
  subroutine pair_correlation(p,R,gr)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: R(p%dim,p%Np)
    real(8), intent(inout) :: gr(p%Nbin)
    real(8) :: x(p%dim),r2
    integer :: i,j,ibin
    do i=1,p%Np-1
       do j=i+1,p%Np
          x  = R(:,i)-R(:,j)
          r2 = image_r2(p,x)
          if (r2<=p%rcut2) then
             ibin     = int(sqrt(r2)/p%rbin)+1
             gr(ibin) = gr(ibin)+2.d0
          end if
       end do
    end do
  end subroutine pair_correlation

  ! S(k) along the box axes, k = iq*2pi/L
  subroutine structure_factor(p,R,Sk)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: R(p%dim,p%Np)
    real(8), intent(inout) :: Sk(p%dim,p%Nk)
    real(8) :: c,s,qr
    integer :: iq,k,i
    do iq=1,p%Nk
       do k=1,p%dim
          c = 0.d0
          s = 0.d0
          do i=1,p%Np
             qr = real(iq)*p%qbin(k)*R(k,i)
             c  = c+cos(qr)
             s  = s+sin(qr)
          end do
          Sk(k,iq) = Sk(k,iq)+(c*c+s*s)
       end do
    end do
  end subroutine structure_factor

  ! one-body density matrix histogram of the worm's end-to-end vector, with 2m partial waves
  subroutine obdm_accumulate(p,xend,nrho)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: xend(p%dim,2)
    real(8), intent(inout) :: nrho(0:p%Npw,p%Nbin)
    real(8) :: x(p%dim),r2,r
    complex(8) :: e1,e2,em
    integer :: ibin,m
    x  = xend(:,1)-xend(:,2)
    r2 = image_r2(p,x)
    if (r2<=p%rcut2) then
       r    = sqrt(r2)
       ibin = int(r/p%rbin)+1
       e1   = cmplx(x(1)/r,x(2)/r,8)
       e2   = e1*e1
       em   = 1.d0
       do m=0,p%Npw
          nrho(m,ibin) = nrho(m,ibin)+real(em)
          em = em*e2
       end do
    end if
  end subroutine obdm_accumulate

  ! volume of the unit d-ball
  function unit_ball(p) result(kn)
    type(est_params), intent(in) :: p
    real(8) :: kn
    kn = p%pi**(0.5d0*p%dim)/gamma(0.5d0*p%dim+1.d0)
  end function unit_ball

  subroutine normalize_gr(p,density,ngr,gr)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: density
    integer, intent(in)    :: ngr
    real(8), intent(inout) :: gr(p%Nbin)
    real(8) :: kn,norm,r,nid
    integer :: ibin
    kn   = unit_ball(p)
    norm = real(p%Np)*real(ngr)
    do ibin=1,p%Nbin
       r   = (real(ibin)-0.5d0)*p%rbin
       nid = density*kn*((r+0.5d0*p%rbin)**p%dim-(r-0.5d0*p%rbin)**p%dim)
       gr(ibin) = gr(ibin)/(nid*norm)
    end do
  end subroutine normalize_gr

  subroutine normalize_sk(p,ngr,Sk)
    type(est_params), intent(in) :: p
    integer, intent(in)    :: ngr
    real(8), intent(inout) :: Sk(p%dim,p%Nk)
    real(8) :: norm
    norm = real(p%Np)*real(ngr)
    Sk = Sk/norm
  end subroutine normalize_sk

  subroutine normalize_nr(p,density,zconf,Nobdm,nrho)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: density,zconf
    integer, intent(in)    :: Nobdm
    real(8), intent(inout) :: nrho(0:p%Npw,p%Nbin)
    real(8) :: kn,r,nid
    integer :: ibin
    kn = unit_ball(p)
    do ibin=1,p%Nbin
       r   = (real(ibin)-0.5d0)*p%rbin
       nid = density*kn*((r+0.5d0*p%rbin)**p%dim-(r-0.5d0*p%rbin)**p%dim)
       nrho(:,ibin) = nrho(:,ibin)/(p%CWorm*nid*zconf*real(Nobdm))
    end do
  end subroutine normalize_nr

  ! ---- density profiles of a trapped system (counts of pigs_density_read: slice Nb, grid half-width h, Nbin bins per
  ! axis) -> one walker's profiles of one block with S samples: planar c/(S b^min(dim,2)) over [-h,h) with b = (2h)/Nbin,
  ! radial c/(S dV_j) and pair c/(S Np dV_j) over [0,h) with br = h/Nbin and dV_j = V_d(j br) - V_d((j-1) br).
  ! With every particle inside the grid the planar and radial profiles integrate to Np, the pair distribution to Np-1.
  subroutine normalize_density(dim,Np,Nbin,h,S,cpl,crad,cpair,dpl,drad,dpair)
    integer, intent(in)    :: dim,Np,Nbin
    real(8), intent(in)    :: h
    integer(8), intent(in) :: S,cpl(:),crad(Nbin),cpair(Nbin)
    real(8), intent(out)   :: dpl(:),drad(Nbin),dpair(Nbin)
    real(8) :: b,br,kn,dv
    integer :: j
    b  = (2.d0*h)/Nbin
    br = h/Nbin
    kn = acos(-1.d0)**(0.5d0*dim)/gamma(0.5d0*dim+1.d0)
    dpl = real(cpl,8)/(real(S,8)*b**min(dim,2))
    do j=1,Nbin
       dv       = kn*(real(j,8)*br)**dim-kn*(real(j-1,8)*br)**dim
       drad(j)  = real(crad(j),8)/(real(S,8)*dv)
       dpair(j) = real(cpair(j),8)/(real(S,8)*real(Np,8)*dv)
    end do
  end subroutine normalize_density

  ! dens_vpi.out: x y mean err with x fastest and a blank line after each y row (dim >= 2), x mean err (dim = 1); bin
  ! centres of the planar grid
  subroutine write_density(fname,dim,Nbin,h,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: dim,Nbin,n
    real(8), intent(in)    :: h
    real(8), intent(inout) :: av(:),av2(:)
    real(8) :: b,x,y
    integer :: i,j1,j2,u
    b = (2.d0*h)/Nbin
    av  = av/real(n)
    av2 = av2/real(n)
    open (newunit=u,file=fname)
    if (dim==1) then
       do j1=1,Nbin
          x = -h+(real(j1)-0.5d0)*b
          write (u,'(20g20.10e3)') x,av(j1),variance(n,av(j1),av2(j1))
       end do
    else
       do j2=1,Nbin
          y = -h+(real(j2)-0.5d0)*b
          do j1=1,Nbin
             x = -h+(real(j1)-0.5d0)*b
             i = j1+Nbin*(j2-1)
             write (u,'(20g20.10e3)') x,y,av(i),variance(n,av(i),av2(i))
          end do
          write (u,'(a)') ''
       end do
    end if
    close (u)
  end subroutine write_density

  ! rho_vpi.out / pr_vpi.out: r mean err at the bin centres of [0,h), br = h/Nbin
  subroutine write_profile(fname,Nbin,h,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: Nbin,n
    real(8), intent(in)    :: h
    real(8), intent(inout) :: av(Nbin),av2(Nbin)
    real(8) :: br,r
    integer :: j,u
    br = h/Nbin
    open (newunit=u,file=fname)
    do j=1,Nbin
       r      = (real(j)-0.5d0)*br
       av(j)  = av(j)/real(n)
       av2(j) = av2(j)/real(n)
       write (u,'(20g20.10e3)') r,av(j),variance(n,av(j),av2(j))
    end do
    close (u)
  end subroutine write_profile

  ! ---- imaginary-time density correlations (raw sums of pigs_fqt_read: window slices Nb-window..Nb+window, lags
  ! 0..Ntau) -> one walker's F(q,tau_l) of one block with S samples: raw/(S n_pairs(l) Np), n_pairs(l) = 2 window + 1 - l
  ! products per sample.  Lag 0 is S(k) averaged over the window (window = 0: normalize_sk's value).
  subroutine normalize_fqt(p,Ntau,window,S,raw,F)
    type(est_params), intent(in) :: p
    integer, intent(in)    :: Ntau,window
    integer(8), intent(in) :: S
    real(8), intent(in)    :: raw(p%dim,p%Nk,0:Ntau)
    real(8), intent(out)   :: F(p%dim,p%Nk,0:Ntau)
    integer :: l
    do l=0,Ntau
       F(:,:,l) = raw(:,:,l)/(real(S,8)*real(2*window+1-l,8)*real(p%Np,8))
    end do
  end subroutine normalize_fqt

  ! fqt_vpi.out: one table per lag laid out like sk_vpi.out (q, mean, err per axis), each preceded by a comment line
  ! with l, tau_l = l dt and n_pairs(l), and followed by two blank lines (a gnuplot index)
  subroutine write_fqt(fname,p,Ntau,window,dt,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in)    :: Ntau,window,n
    real(8), intent(in)    :: dt
    real(8), intent(inout) :: av(p%dim,p%Nk,0:Ntau),av2(p%dim,p%Nk,0:Ntau)
    integer :: j,k,l,u
    open (newunit=u,file=fname)
    do l=0,Ntau
       write (u,'(a,i6,a,g20.10e3,a,i6)') '# l =',l,'  tau =',real(l,8)*dt,'  n_pairs =',2*window+1-l
       do j=1,p%Nk
          av(:,j,l)  = av(:,j,l)/real(n)
          av2(:,j,l) = av2(:,j,l)/real(n)
          write (u,'(20g20.10e3)') (j*p%qbin(k),av(k,j,l),variance(n,av(k,j,l),av2(k,j,l)),k=1,p%dim)
       end do
       write (u,'(a)') ''
       write (u,'(a)') ''
    end do
    close (u)
  end subroutine write_fqt

  ! ---- imaginary-time profiles (raw sums of pigs_tau_read: Vpair, Vext, W = sum r v'(r), D2 = sum_i |x_i(b)-x_i(b+1)|^2 of
  ! every slice b = 0..2Nb) -> one walker's profiles of one block with S samples, per particle: T(1:3,b) = raw(1:3,b)/(S Np)
  ! and the kinetic estimator of the link b -> b+1, T(4,b) = dim/(2 dt) - D2(b)/(2 dt^2 Np S) (b = 2Nb has no link: 0)
  subroutine normalize_tau(dim,Np,Nb,dt,S,raw,T)
    integer, intent(in)    :: dim,Np,Nb
    real(8), intent(in)    :: dt
    integer(8), intent(in) :: S
    real(8), intent(in)    :: raw(4,0:2*Nb)
    real(8), intent(out)   :: T(4,0:2*Nb)
    integer :: b
    do b=0,2*Nb
       T(1:3,b) = raw(1:3,b)/(real(S,8)*real(Np,8))
       T(4,b)   = real(dim,8)/(2.d0*dt)-raw(4,b)/(2.d0*dt*dt*real(Np,8)*real(S,8))
    end do
    T(4,2*Nb) = 0.d0
  end subroutine normalize_tau

  ! tau_vpi.out: one row per slice: b, tau_b = (b-Nb) dt, then mean and error of Vpair/Np, Vext/Np, W/Np and of the link's
  ! kinetic estimator (left out in the last row: slice 2Nb starts no link)
  subroutine write_tau(fname,Nb,dt,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: Nb,n
    real(8), intent(in)    :: dt
    real(8), intent(inout) :: av(4,0:2*Nb),av2(4,0:2*Nb)
    integer :: b,k,u,nc
    open (newunit=u,file=fname)
    do b=0,2*Nb
       av(:,b)  = av(:,b)/real(n)
       av2(:,b) = av2(:,b)/real(n)
       nc = merge(3,4,b==2*Nb)
       write (u,'(20g20.10e3)') real(b,8),real(b-Nb,8)*dt,(av(k,b),variance(n,av(k,b),av2(k,b)),k=1,nc)
    end do
    close (u)
  end subroutine write_tau

  ! ---- bond-orientational order (raw sums and counts of pigs_bop_read over the window slices Nb-window..Nb+window) -> one
  ! walker's block values with S samples, n = S (2 window + 1) slices: B = Q4, Q6, the particle means of q4(i) and q6(i),
  ! each per slice, and the coordination sum n_i/(Np n); P(:,l) the distributions of q4(i), q6(i) as probability densities
  ! on [0,1] (counts Nh/(n Np)); G6 = G/GN per radial bin (0 in a bin that held no pair in this block)
  subroutine normalize_bop(Np,window,S,Nh,Nr,rawS,H,G,GN,B,P,G6)
    integer, intent(in)    :: Np,window,Nh,Nr
    integer(8), intent(in) :: S
    real(8), intent(in)    :: rawS(8),G(Nr)
    integer(8), intent(in) :: H(Nh,2),GN(Nr)
    real(8), intent(out)   :: B(5),P(Nh,2),G6(Nr)
    real(8) :: n
    integer :: j
    n = real(S,8)*real(2*window+1,8)
    B(1) = rawS(1)/n; B(2) = rawS(3)/n; B(3) = rawS(5)/n; B(4) = rawS(6)/n
    B(5) = rawS(7)/(n*real(Np,8))
    P = real(H,8)*real(Nh,8)/(n*real(Np,8))
    do j=1,Nr
       G6(j) = 0.d0
       if (GN(j)>0) G6(j) = G(j)/real(GN(j),8)
    end do
  end subroutine normalize_bop

  ! bo_vpi.out: one row: mean and error of Q4, Q6, <q4(i)>, <q6(i)> and the coordination
  subroutine write_bo(fname,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: n
    real(8), intent(inout) :: av(5),av2(5)
    integer :: k,u
    open (newunit=u,file=fname)
    av  = av/real(n)
    av2 = av2/real(n)
    write (u,'(20g20.10e3)') (av(k),variance(n,av(k),av2(k)),k=1,5)
    close (u)
  end subroutine write_bo

  ! boh_vpi.out: one row per bin of [0,1]: centre, then mean and error of P(q4) and of P(q6)
  subroutine write_boh(fname,Nh,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: Nh,n
    real(8), intent(inout) :: av(Nh,2),av2(Nh,2)
    integer :: j,k,u
    open (newunit=u,file=fname)
    av  = av/real(n)
    av2 = av2/real(n)
    do j=1,Nh
       write (u,'(20g20.10e3)') (real(j,8)-0.5d0)/real(Nh,8),(av(j,k),variance(n,av(j,k),av2(j,k)),k=1,2)
    end do
    close (u)
  end subroutine write_boh

  ! ---- vector structure factor on the full reciprocal grid (raw sums of pigs_sqv_read: window slices
  ! Nb-window..Nb+window) -> one walker's S(q) of one block with S samples: raw/(S (2 window + 1) Np)
  subroutine normalize_sqv(Np,window,S,Nq,raw,Sq)
    integer, intent(in)    :: Np,window,Nq
    integer(8), intent(in) :: S
    real(8), intent(in)    :: raw(Nq)
    real(8), intent(out)   :: Sq(Nq)
    Sq = raw/(real(S,8)*real(2*window+1,8)*real(Np,8))
  end subroutine normalize_sqv

  ! The |q| shells of the stored vectors nv(dim,Nq): shell(iqv) = 1..nsh in ascending |q|, qsh the modulus (root of the
  ! shell's mean |q|^2) and mult the multiplicity counting +q and -q.  With all box lengths bitwise equal the shell key
  ! is the integer sum of n_k^2; otherwise vectors whose |q|^2 agree to 1e-12 relative share a shell.
  subroutine sqv_shells(p,Nq,nv,shell,nsh,qsh,mult)
    type(est_params), intent(in) :: p
    integer, intent(in)  :: Nq
    integer(4), intent(in) :: nv(p%dim,Nq)
    integer, intent(out) :: shell(Nq),nsh
    real(8), allocatable, intent(out) :: qsh(:)
    integer, allocatable, intent(out) :: mult(:)
    real(8) :: key(Nq),q2(Nq),qs(Nq)
    integer :: idx(Nq),tmp(Nq),cnt(Nq),i,k
    logical :: cubic
    cubic = .true.
    do k=2,p%dim
       cubic = cubic .and. p%Lbox(k)==p%Lbox(1)
    end do
    do i=1,Nq
       q2(i) = 0.d0; key(i) = 0.d0
       do k=1,p%dim
          q2(i)  = q2(i)+(real(nv(k,i),8)*p%qbin(k))**2
          key(i) = key(i)+real(nv(k,i),8)**2
       end do
       if (.not. cubic) key(i) = q2(i)
       idx(i) = i
    end do
    call msort(1,Nq)
    nsh = 0; cnt = 0; qs = 0.d0
    do i=1,Nq
       if (i==1) then
          nsh = 1
       else if (key(idx(i))-key(idx(i-1))>1.d-12*key(idx(i))) then
          nsh = nsh+1
       end if
       shell(idx(i)) = nsh
       cnt(nsh) = cnt(nsh)+1
       qs(nsh)  = qs(nsh)+q2(idx(i))
    end do
    allocate (qsh(nsh),mult(nsh))
    qsh  = sqrt(qs(1:nsh)/cnt(1:nsh))
    mult = 2*cnt(1:nsh)
  contains
    ! stable merge sort of idx(lo:hi) by key
    recursive subroutine msort(lo,hi)
      integer, intent(in) :: lo,hi
      integer :: mid,a,b,c
      if (hi<=lo) return
      mid = (lo+hi)/2
      call msort(lo,mid); call msort(mid+1,hi)
      a = lo; b = mid+1
      do c=lo,hi
         if (b>hi) then
            tmp(c) = idx(a); a = a+1
         else if (a>mid) then
            tmp(c) = idx(b); b = b+1
         else if (key(idx(b))<key(idx(a))) then
            tmp(c) = idx(b); b = b+1
         else
            tmp(c) = idx(a); a = a+1
         end if
      end do
      idx(lo:hi) = tmp(lo:hi)
    end subroutine msort
  end subroutine sqv_shells

  ! C-callable handle on sqv_shells (no state): Lbox(dim) as the front end holds it, qbin = 2 pi / Lbox as it sets it
  ! (pigs_vpi.f90); qsh and mult hold the first nsh of Nq entries.  For tests of the host logic.
  subroutine est_sqv_shells(dim,Lbox,Nq,nv,shell,nsh,qsh,mult) bind(C,name='est_sqv_shells')
    use iso_c_binding
    integer(c_int), value :: dim,Nq
    real(c_double), intent(in) :: Lbox(dim)
    integer(c_int32_t), intent(in) :: nv(dim,Nq)
    integer(c_int), intent(out) :: shell(Nq),nsh,mult(Nq)
    real(c_double), intent(out) :: qsh(Nq)
    type(est_params) :: p
    real(8), allocatable :: q(:)
    integer, allocatable :: m(:)
    p%dim = dim; p%pi = acos(-1.d0)
    p%Lbox = 1.d0; p%Lbox(1:dim) = Lbox; p%LboxHalf = 0.5d0*p%Lbox; p%qbin = 2.d0*p%pi/p%Lbox
    call sqv_shells(p,Nq,nv,shell,nsh,q,m)
    qsh(1:nsh) = q; mult(1:nsh) = m
  end subroutine est_sqv_shells

  ! mean of Sq over the stored vectors of every shell
  subroutine sqv_shell_means(Nq,shell,nsh,mult,Sq,Ssh)
    integer, intent(in)  :: Nq,nsh,shell(Nq),mult(nsh)
    real(8), intent(in)  :: Sq(Nq)
    real(8), intent(out) :: Ssh(nsh)
    integer :: i
    Ssh = 0.d0
    do i=1,Nq
       Ssh(shell(i)) = Ssh(shell(i))+Sq(i)
    end do
    Ssh = Ssh/(0.5d0*real(mult,8))
  end subroutine sqv_shell_means

  ! sqvec_vpi.out: one line per stored vector: n_1..n_dim, |q|, S(q), error over the n blocks
  subroutine write_sqvec(fname,p,Nq,nv,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in)    :: Nq,n
    integer(4), intent(in) :: nv(p%dim,Nq)
    real(8), intent(inout) :: av(Nq),av2(Nq)
    integer :: i,k,u
    real(8) :: q2
    character(len=24) :: fmt
    write (fmt,'(a,i0,a)') '(',p%dim,'i6,3g20.10e3)'
    open (newunit=u,file=fname)
    do i=1,Nq
       av(i)  = av(i)/real(n)
       av2(i) = av2(i)/real(n)
       q2 = 0.d0
       do k=1,p%dim
          q2 = q2+(real(nv(k,i),8)*p%qbin(k))**2
       end do
       write (u,fmt) (nv(k,i),k=1,p%dim),sqrt(q2),av(i),variance(n,av(i),av2(i))
    end do
    close (u)
  end subroutine write_sqvec

  ! sq_vpi.out: one line per |q| shell: |q|, S, error over the n blocks, multiplicity (+q and -q)
  subroutine write_sqshell(fname,nsh,qsh,mult,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: nsh,mult(nsh),n
    real(8), intent(in)    :: qsh(nsh)
    real(8), intent(inout) :: av(nsh),av2(nsh)
    integer :: i,u
    open (newunit=u,file=fname)
    do i=1,nsh
       av(i)  = av(i)/real(n)
       av2(i) = av2(i)/real(n)
       write (u,'(3g20.10e3,i8)') qsh(i),av(i),variance(n,av(i),av2(i)),mult(i)
    end do
    close (u)
  end subroutine write_sqshell

  ! ---- F(q,tau) on the full reciprocal grid (raw sums of pigs_fqv_read: the vectors of the vector S(q), window slices
  ! Nb-window..Nb+window, lags 0..Ntau) -> one walker's F(q,tau_l) of one block with S samples:
  ! raw/(S n_pairs(l) Np), n_pairs(l) = 2 window + 1 - l.  Lag 0 is normalize_sqv's value.
  subroutine normalize_fqv(Np,Ntau,window,S,Nq,raw,F)
    integer, intent(in)    :: Np,Ntau,window,Nq
    integer(8), intent(in) :: S
    real(8), intent(in)    :: raw(Nq,0:Ntau)
    real(8), intent(out)   :: F(Nq,0:Ntau)
    integer :: l
    do l=0,Ntau
       F(:,l) = raw(:,l)/(real(S,8)*real(2*window+1-l,8)*real(Np,8))
    end do
  end subroutine normalize_fqv

  ! fqvec_vpi.out: one line per (lag, stored vector), lags slowest: l, tau_l = l dt, n_1..n_dim, |q|, F, error over the
  ! n blocks
  subroutine write_fqvec(fname,p,Ntau,dt,Nq,nv,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in)    :: Ntau,Nq,n
    real(8), intent(in)    :: dt
    integer(4), intent(in) :: nv(p%dim,Nq)
    real(8), intent(inout) :: av(Nq,0:Ntau),av2(Nq,0:Ntau)
    integer :: i,k,l,u
    real(8) :: q2
    character(len=32) :: fmt
    write (fmt,'(a,i0,a)') '(i6,g20.10e3,',p%dim,'i6,3g20.10e3)'
    open (newunit=u,file=fname)
    do l=0,Ntau
       do i=1,Nq
          av(i,l)  = av(i,l)/real(n)
          av2(i,l) = av2(i,l)/real(n)
          q2 = 0.d0
          do k=1,p%dim
             q2 = q2+(real(nv(k,i),8)*p%qbin(k))**2
          end do
          write (u,fmt) l,real(l,8)*dt,(nv(k,i),k=1,p%dim),sqrt(q2),av(i,l),variance(n,av(i,l),av2(i,l))
       end do
    end do
    close (u)
  end subroutine write_fqvec

  ! fqsh_vpi.out: one line per (lag, |q| shell), lags slowest: l, tau_l, |q|, F, error over the n blocks, multiplicity
  ! (+q and -q); the shells are sq_vpi.out's
  subroutine write_fqshell(fname,Ntau,dt,nsh,qsh,mult,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: Ntau,nsh,mult(nsh),n
    real(8), intent(in)    :: dt,qsh(nsh)
    real(8), intent(inout) :: av(nsh,0:Ntau),av2(nsh,0:Ntau)
    integer :: i,l,u
    open (newunit=u,file=fname)
    do l=0,Ntau
       do i=1,nsh
          av(i,l)  = av(i,l)/real(n)
          av2(i,l) = av2(i,l)/real(n)
          write (u,'(i6,4g20.10e3,i8)') l,real(l,8)*dt,qsh(i),av(i,l),variance(n,av(i,l),av2(i,l)),mult(i)
       end do
    end do
    close (u)
  end subroutine write_fqshell

  ! ---- imaginary-time displacement (raw sums D of pigs_fqs_read: r^2 and r^4 of the once-folded x_i(a+l) - x_i(a) over
  ! the pairs of the window slices and the particles) -> one walker's block values with S samples: m(1,l) = <dr^2>(tau_l),
  ! m(2,l) = <dr^4>(tau_l), each raw/(S n_pairs(l) Np).  The self part F_s of the same call goes through normalize_fqv.
  subroutine normalize_msd(Np,Ntau,window,S,raw,m)
    integer, intent(in)    :: Np,Ntau,window
    integer(8), intent(in) :: S
    real(8), intent(in)    :: raw(2,0:Ntau)
    real(8), intent(out)   :: m(2,0:Ntau)
    integer :: l
    do l=0,Ntau
       m(:,l) = raw(:,l)/(real(S,8)*real(2*window+1-l,8)*real(Np,8))
    end do
  end subroutine normalize_msd

  ! msd_vpi.out: one line per lag: l, tau_l = l dt, <dr^2>, its error over the n blocks, and the non-Gaussian parameter
  ! alpha_2 = dim <dr^4> / ((dim + 2) <dr^2>^2) - 1 of the averaged moments (0 where <dr^2> is 0: lag 0)
  subroutine write_msd(fname,dim,Ntau,dt,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: dim,Ntau,n
    real(8), intent(in)    :: dt
    real(8), intent(inout) :: av(2,0:Ntau),av2(2,0:Ntau)
    integer :: l,u
    real(8) :: a2
    open (newunit=u,file=fname)
    do l=0,Ntau
       av(:,l)  = av(:,l)/real(n)
       av2(:,l) = av2(:,l)/real(n)
       a2 = 0.d0
       if (av(1,l)>0.d0) a2 = real(dim,8)*av(2,l)/(real(dim+2,8)*av(1,l)*av(1,l))-1.d0
       write (u,'(i6,4g20.10e3)') l,real(l,8)*dt,av(1,l),variance(n,av(1,l),av2(1,l)),a2
    end do
    close (u)
  end subroutine write_msd

  ! ---- pair distribution on the vector grid over a slice window (counts of pigs_grv_read: window slices
  ! Nb-window..Nb+window, Ng bins per axis over the minimum-image cell, nv = Ng**dim, x fastest; radial counts on the run's
  ! own Nbin/rbin grid) -> one walker's block values with S samples.  The device counts the ordered pair i < j only: the
  ! partner -d is the reflected bin nv+1-j, and g = (c(j) + c(nv+1-j))/(S (2 window + 1) Np density prod_k b_k), which is
  ! 1 - 1/Np for an ideal gas.  The radial part is the reference's g(r): 2 per pair through normalize_gr with
  ! S (2 window + 1) slices, so at window 0 it is gr_vpi.out's.
  subroutine normalize_grv(p,density,window,S,Ng,nv,cvec,crad,gvec,grw)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: density
    integer, intent(in)    :: window,Ng,nv
    integer(8), intent(in) :: S,cvec(nv),crad(p%Nbin)
    real(8), intent(out)   :: gvec(nv),grw(p%Nbin)
    real(8) :: cell
    integer :: j,k
    cell = 1.d0
    do k=1,p%dim
       cell = cell*(p%Lbox(k)/real(Ng,8))
    end do
    do j=1,nv
       gvec(j) = real(cvec(j)+cvec(nv+1-j),8)/(real(S,8)*real(2*window+1,8)*real(p%Np,8)*density*cell)
    end do
    grw = 2.d0*real(crad,8)
    call normalize_gr(p,density,int(S)*(2*window+1),grw)
  end subroutine normalize_grv

  ! ---- van Hove functions over a slice window (counts of pigs_vh_read: lags 0..Ntau between the window slices
  ! Nb-window..Nb+window; the distinct part on the radial grid of p (Nbin, rbin), the self part on that of ps) -> one
  ! walker's block values with S samples.  Lag l has 2 window + 1 - l slice pairs, and both parts go through normalize_gr
  ! with S (2 window + 1 - l) of them: G_d = dist/(S n_pairs Np density dV), which at l = 0 is grw_vpi.out's g(r) (the
  ! device counts the ordered pairs i /= j, twice the pairs i < j), and G_s = self/(S n_pairs Np dV), density 1.
  subroutine normalize_vh(p,ps,density,window,S,Ntau,cself,cdist,gs,gd)
    type(est_params), intent(in) :: p,ps
    real(8), intent(in)    :: density
    integer, intent(in)    :: window,Ntau
    integer(8), intent(in) :: S,cself(ps%Nbin,0:Ntau),cdist(p%Nbin,0:Ntau)
    real(8), intent(out)   :: gs(ps%Nbin,0:Ntau),gd(p%Nbin,0:Ntau)
    integer :: l
    gd = real(cdist,8)
    gs = real(cself,8)
    do l=0,Ntau
       call normalize_gr(p,density,int(S)*(2*window+1-l),gd(:,l))
       call normalize_gr(ps,1.d0,int(S)*(2*window+1-l),gs(:,l))
    end do
  end subroutine normalize_vh

  ! gd_vpi.out, gs_vpi.out: one line per (lag, bin), lags outermost: tau_l = l dt, r at the bin centre, G, error over the n blocks
  subroutine write_vh(fname,p,dt,Ntau,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: dt
    integer, intent(in)    :: Ntau,n
    real(8), intent(inout) :: av(p%Nbin,0:Ntau),av2(p%Nbin,0:Ntau)
    integer :: j,l,u
    open (newunit=u,file=fname)
    av  = av/real(n)
    av2 = av2/real(n)
    do l=0,Ntau
       do j=1,p%Nbin
          write (u,'(20g20.10e3)') real(l,8)*dt,(real(j)-0.5d0)*p%rbin,av(j,l),variance(n,av(j,l),av2(j,l))
       end do
    end do
    close (u)
  end subroutine write_vh

  ! ---- triplet distribution over a slice window (counts of pigs_g3_read on the radial grid of p, Nbin = Nr bins of rbin, and
  ! Na bins of cos(theta) on [-1,1]; trip on the packed upper triangle of the leg bins lo <= hi, rows lo) -> one walker's
  ! block values with S samples, St = S (2 window + 1), vol(b) the shell volume of normalize_gr:
  !   g2(b)       = pair/(St Np density vol(b))
  !   g3(q,lo,hi) = trip/(St Np density^2 vol(lo) vol(hi) w(q) m),  m = 1 for lo < hi and 1/2 for lo = hi,
  !   w(q) = 1/Na in 3D and (acos(c_q) - acos(c_q+1))/pi in 2D, c_q = -1 + 2 q/Na
  !   pang(q)     = P(cos theta) of all pairs of legs, normalised to integrate to 1 over [-1,1]; 0 without triplets
  subroutine normalize_g3(p,density,window,S,Na,ctrip,cpair,g2,g3,pang)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: density
    integer, intent(in)    :: window,Na
    integer(8), intent(in) :: S,ctrip(Na,p%Nbin*(p%Nbin+1)/2),cpair(p%Nbin)
    real(8), intent(out)   :: g2(p%Nbin),g3(Na,p%Nbin*(p%Nbin+1)/2),pang(Na)
    real(8) :: kn,St,r,vol(p%Nbin),w(Na),m,tot,c0,c1
    integer :: b,lo,hi,q,k
    kn = unit_ball(p)
    St = real(S,8)*real(2*window+1,8)
    do b=1,p%Nbin
       r      = (real(b,8)-0.5d0)*p%rbin
       vol(b) = kn*((r+0.5d0*p%rbin)**p%dim-(r-0.5d0*p%rbin)**p%dim)
       g2(b)  = real(cpair(b),8)/(St*real(p%Np,8)*density*vol(b))
    end do
    do q=1,Na
       if (p%dim==3) then
          w(q) = 1.d0/real(Na,8)
       else
          c0   = max(-1.d0,min(1.d0,-1.d0+2.d0*real(q-1,8)/real(Na,8)))
          c1   = max(-1.d0,min(1.d0,-1.d0+2.d0*real(q,8)/real(Na,8)))
          w(q) = (acos(c0)-acos(c1))/p%pi
       end if
    end do
    k = 0
    pang = 0.d0
    do lo=1,p%Nbin
       do hi=lo,p%Nbin
          k = k+1
          m = merge(0.5d0,1.d0,lo==hi)
          do q=1,Na
             g3(q,k) = real(ctrip(q,k),8)/(St*real(p%Np,8)*density**2*(vol(lo)*vol(hi)*m)*w(q))
             pang(q) = pang(q)+real(ctrip(q,k),8)
          end do
       end do
    end do
    tot = sum(pang)*(2.d0/real(Na,8))
    if (tot>0.d0) pang = pang/tot
  end subroutine normalize_g3

  ! g3_vpi.out: one line per (lo, hi, q), q fastest, in the packed order: r_lo, r_hi and cos(theta) at the bin centres, g3,
  ! error over the n blocks
  subroutine write_g3(fname,p,Na,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in)    :: Na,n
    real(8), intent(inout) :: av(Na,p%Nbin*(p%Nbin+1)/2),av2(Na,p%Nbin*(p%Nbin+1)/2)
    integer :: lo,hi,q,k,u
    open (newunit=u,file=fname)
    av  = av/real(n)
    av2 = av2/real(n)
    k = 0
    do lo=1,p%Nbin
       do hi=lo,p%Nbin
          k = k+1
          do q=1,Na
             write (u,'(20g20.10e3)') (real(lo,8)-0.5d0)*p%rbin,(real(hi,8)-0.5d0)*p%rbin, &
                  & -1.d0+(real(q,8)-0.5d0)*(2.d0/real(Na,8)),av(q,k),variance(n,av(q,k),av2(q,k))
          end do
       end do
    end do
    close (u)
  end subroutine write_g3

  ! g3ang_vpi.out: one line per bin of cos(theta): its centre, P(cos theta), error over the n blocks
  subroutine write_g3ang(fname,Na,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: Na,n
    real(8), intent(inout) :: av(Na),av2(Na)
    integer :: q,u
    open (newunit=u,file=fname)
    av  = av/real(n)
    av2 = av2/real(n)
    do q=1,Na
       write (u,'(20g20.10e3)') -1.d0+(real(q,8)-0.5d0)*(2.d0/real(Na,8)),av(q),variance(n,av(q),av2(q))
    end do
    close (u)
  end subroutine write_g3ang

  ! ---- Axilrod-Teller-Muto three-body energy over a slice window (raw sums T and counts ntrip of pigs_atm_read, one value
  ! per window slice a = Nb-window..Nb+window) -> one walker's block values with S samples and the coupling nu:
  !   B(1,a) = V3/Np of slice a = nu T(a)/(S Np);   B(2,a) = the mean number of triplets within rc = ntrip(a)/S
  subroutine normalize_atm(Np,window,nu,S,T,ntrip,B)
    integer, intent(in)    :: Np,window
    real(8), intent(in)    :: nu,T(-window:window)
    integer(8), intent(in) :: S,ntrip(-window:window)
    real(8), intent(out)   :: B(2,-window:window)
    integer :: a
    do a=-window,window
       B(1,a) = nu*T(a)/(real(S,8)*real(Np,8))
       B(2,a) = real(ntrip(a),8)/real(S,8)
    end do
  end subroutine normalize_atm

  ! V3/Np of the block values B averaged over the window
  function atm_window_mean(window,B) result(v3)
    integer, intent(in) :: window
    real(8), intent(in) :: B(2,-window:window)
    real(8) :: v3
    v3 = sum(B(1,:))/real(2*window+1,8)
  end function atm_window_mean

  ! first line of v3_vpi*.out
  subroutine v3_header(u,window)
    integer, intent(in) :: u,window
    write (u,'(a,i0,a,i0,a)') '# block, V3/Np = nu <sum_{i<j<k} (1 + 3 cos cos cos)/(r r r)^3>/Np over the slices Nb-',window,'..Nb+', &
         & window,' (triplets with a side beyond atm_rc are not counted, no tail correction), P3 = 9 density (V3/Np)/dim'
  end subroutine v3_header

  ! one line of v3_vpi*.out: the block, V3/Np over the window, and its pressure P3 = 9 nu <T>/(dim Volume)
  subroutine write_v3_block(u,iblock,dim,density,v3)
    integer, intent(in) :: u,iblock,dim
    real(8), intent(in) :: density,v3
    write (u,'(20g20.10e3)') real(iblock),v3,9.d0*density*v3/real(dim,8)
  end subroutine write_v3_block

  ! v3tau_vpi.out: one row per window slice a: a, tau_a = (a-Nb) dt, mean and error of V3/Np over the n blocks, and the mean
  ! number of triplets within rc
  subroutine write_v3tau(fname,Nb,window,dt,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in)    :: Nb,window,n
    real(8), intent(in)    :: dt
    real(8), intent(inout) :: av(2,-window:window),av2(2,-window:window)
    integer :: a,u
    open (newunit=u,file=fname)
    av  = av/real(n)
    av2 = av2/real(n)
    do a=-window,window
       write (u,'(20g20.10e3)') real(Nb+a,8),real(a,8)*dt,av(1,a),variance(n,av(1,a),av2(1,a)),av(2,a)
    end do
    close (u)
  end subroutine write_v3tau

  ! ---- momentum distribution (cosine sums C and the sample count nopen of pigs_nk_read) -> one walker's n(k) of one block
  ! in the reference's NormalizeNr convention, zconf the diagonal configurations of the block:
  !   B(0) = n(0) = nopen/(CWorm zconf Nobdm);   B(i) = n(k_i) = C(i)/(CWorm zconf Nobdm);   n0 = B(0)/Np
  subroutine normalize_nk(cworm,zconf,Nobdm,Nq,C,nopen,B)
    real(8), intent(in)    :: cworm,zconf,C(Nq)
    integer, intent(in)    :: Nobdm,Nq
    integer(8), intent(in) :: nopen
    real(8), intent(out)   :: B(0:Nq)
    real(8) :: den
    den = cworm*zconf*real(Nobdm,8)
    B(0)  = real(nopen,8)/den
    B(1:) = C/den
  end subroutine normalize_nk

  ! one-body density matrix over the density per Cartesian bin of the minimum-image cell (counts H of pigs_nk_read, Ng
  ! bins per axis): H/(CWorm zconf Nobdm density bin volume), 1 at r -> 0 like nr_vpi.out
  subroutine normalize_nrvec(p,cworm,zconf,Nobdm,density,Ng,nv,H,R)
    type(est_params), intent(in) :: p
    real(8), intent(in)    :: cworm,zconf,density
    integer, intent(in)    :: Nobdm,Ng,nv
    integer(8), intent(in) :: H(nv)
    real(8), intent(out)   :: R(nv)
    real(8) :: den
    integer :: k
    den = cworm*zconf*real(Nobdm,8)*density
    do k=1,p%dim
       den = den*(p%Lbox(k)/real(Ng,8))
    end do
    R = real(H,8)/den
  end subroutine normalize_nrvec

  ! first line of n0_vpi*.out
  subroutine n0_header(u)
    integer, intent(in) :: u
    write (u,'(a)') '# block, condensate fraction n0 = n(k=0)/Np, n(k=0) = open samples/(CWorm zconf Nobdm)'
  end subroutine n0_header

  ! one line of n0_vpi*.out
  subroutine write_n0_block(u,iblock,Np,nk0)
    integer, intent(in) :: u,iblock,Np
    real(8), intent(in) :: nk0
    write (u,'(20g20.10e3)') real(iblock),nk0/real(Np,8),nk0
  end subroutine write_n0_block

  ! nkvec_vpi.out: one line per vector, n = 0 first and then the stored ones: n_1..n_dim, |k|, n(k), error over the n blocks
  subroutine write_nkvec(fname,p,Nq,nv,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in)    :: Nq,n
    integer(4), intent(in) :: nv(p%dim,Nq)
    real(8), intent(inout) :: av(0:Nq),av2(0:Nq)
    integer :: i,k,u
    real(8) :: q2
    character(len=24) :: fmt
    write (fmt,'(a,i0,a)') '(',p%dim,'i6,3g20.10e3)'
    open (newunit=u,file=fname)
    av  = av/real(n)
    av2 = av2/real(n)
    write (u,fmt) (0,k=1,p%dim),0.d0,av(0),variance(n,av(0),av2(0))
    do i=1,Nq
       q2 = 0.d0
       do k=1,p%dim
          q2 = q2+(real(nv(k,i),8)*p%qbin(k))**2
       end do
       write (u,fmt) (nv(k,i),k=1,p%dim),sqrt(q2),av(i),variance(n,av(i),av2(i))
    end do
    close (u)
  end subroutine write_nkvec

  ! ---- a crystal seen from its lattice (raw sums of pigs_lat_read of one walker and block, S samples) -> the block values
  !   BL(1:7)    = <u^2> over the window, gamma = sqrt(<u^2>)/ann, alpha_2 = dim <u^4>/((dim+2) <u^2>^2) - 1, the vacant
  !                fraction, the multiply occupied fraction, hops per particle and link, hops per particle across the window
  !   BT(:,a)    = <u^2>(tau_a), <u_k^2>(tau_a) k = 1..dim, gamma(tau_a)           (per window slice)
  !   BU(1:nbin) = rho_site(r) = hr/(S ns nsite shell volume);  BU(nbin + (k-1) 2 nbin + b) = P(u_k) = hx(b,k)/(N rbin)
  ! with N the assigned particles of the window (profiles.normalize_lat has the same expressions)
  subroutine normalize_lat(dim,Np,nsite,window,nbin,ann,rmax,pi,S,mom,nass,occ,hr,hx,hop1,hopw,BL,BT,BU)
    integer, intent(in)    :: dim,Np,nsite,window,nbin
    real(8), intent(in)    :: ann,rmax,pi,mom(2+dim,2*window+1)
    integer(8), intent(in) :: S,nass(2*window+1),occ(4,2*window+1),hr(nbin),hx(2*nbin,dim),hop1,hopw
    real(8), intent(out)   :: BL(7),BT(2+dim,2*window+1),BU(nbin*(1+2*dim))
    integer :: a,b,k,ns
    real(8) :: ntot,u2,u4,sites,rbin,shell,lo,hi
    ns = 2*window+1
    do a=1,ns
       BT(1,a) = mom(1,a)/real(nass(a),8)
       do k=1,dim
          BT(1+k,a) = mom(2+k,a)/real(nass(a),8)
       end do
       BT(2+dim,a) = sqrt(BT(1,a))/ann
    end do
    ntot  = real(sum(nass),8)
    u2    = sum(mom(1,:))/ntot
    u4    = sum(mom(2,:))/ntot
    sites = real(S,8)*real(ns,8)*real(nsite,8)
    BL(1) = u2
    BL(2) = sqrt(u2)/ann
    BL(3) = real(dim,8)*u4/(real(dim+2,8)*u2*u2)-1.d0
    BL(4) = real(sum(occ(1,:)),8)/sites
    BL(5) = real(sum(occ(3,:))+sum(occ(4,:)),8)/sites
    BL(6) = 0.d0
    if (ns>1) BL(6) = real(hop1,8)/(real(S,8)*real(Np,8)*real(ns-1,8))
    BL(7) = real(hopw,8)/(real(S,8)*real(Np,8))
    rbin = rmax/real(nbin,8)
    do b=1,nbin
       lo = real(b-1,8)*rbin; hi = real(b,8)*rbin
       if (dim==2) then
          shell = pi*(hi**2-lo**2)
       else
          shell = 4.d0*pi/3.d0*(hi**3-lo**3)
       end if
       BU(b) = real(hr(b),8)/(sites*shell)
    end do
    do k=1,dim
       do b=1,2*nbin
          BU(nbin+(k-1)*2*nbin+b) = real(hx(b,k),8)/(ntot*rbin)
       end do
    end do
  end subroutine normalize_lat

  ! the shortest minimum-image distance between two of the sites R(dim,nsite) in the box (huge for a single site)
  function lat_nn_distance(dim,nsite,R,Lbox) result(ann)
    integer, intent(in) :: dim,nsite
    real(8), intent(in) :: R(dim,nsite),Lbox(dim)
    real(8) :: ann,d,r2
    integer :: i,j,k
    ann = huge(1.d0)
    do i=1,nsite-1
       do j=i+1,nsite
          r2 = 0.d0
          do k=1,dim
             d  = R(k,j)-R(k,i)
             d  = d-Lbox(k)*anint(d/Lbox(k))
             r2 = r2+d*d
          end do
          ann = min(ann,r2)
       end do
    end do
    if (nsite>1) ann = sqrt(ann)
  end function lat_nn_distance

  ! first line of lind_vpi*.out
  subroutine lind_header(u,window)
    integer, intent(in) :: u,window
    write (u,'(a,i0,a,i0,a)') '# block, <u^2> over the slices Nb-',window,'..Nb+',window, &
         & ', Lindemann ratio sqrt(<u^2>)/a_nn, alpha_2, vacant fraction, multiply occupied fraction, hops per particle and link, hops per particle across the window'
  end subroutine lind_header

  ! one line of lind_vpi*.out
  subroutine write_lind_block(u,iblock,BL)
    integer, intent(in) :: u,iblock
    real(8), intent(in) :: BL(7)
    write (u,'(20g20.10e3)') real(iblock),BL
  end subroutine write_lind_block

  ! lindtau_vpi.out: one row per window slice: tau_a = (a-Nb) dt, then the means over the n blocks of <u^2>, <u_k^2> and gamma
  subroutine write_lindtau(fname,dim,window,dt,n,av)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: dim,window,n
    real(8), intent(in) :: dt,av(2+dim,-window:window)
    integer :: a,u
    open (newunit=u,file=fname)
    do a=-window,window
       write (u,'(20g20.10e3)') real(a,8)*dt,av(:,a)/real(n,8)
    end do
    close (u)
  end subroutine write_lindtau

  ! usite_vpi.out: one row per bin b: r at the bin centre, rho_site(r), then per axis k P(u_k = -r) and P(u_k = +r), means
  ! over the n blocks
  subroutine write_usite(fname,dim,nbin,rmax,n,av)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: dim,nbin,n
    real(8), intent(in) :: rmax,av(nbin*(1+2*dim))
    integer :: b,k,u
    open (newunit=u,file=fname)
    do b=1,nbin
       write (u,'(20g20.10e3)') (real(b,8)-0.5d0)*rmax/real(nbin,8),av(b)/real(n,8), &
            & (av(nbin+(k-1)*2*nbin+nbin+1-b)/real(n,8),av(nbin+(k-1)*2*nbin+nbin+b)/real(n,8),k=1,dim)
    end do
    close (u)
  end subroutine write_usite

  ! ---- the superfluid fraction from the centre-of-mass diffusion along tau (raw sums C, D of pigs_sf_read of one walker
  ! and block, S samples) -> the block values per lag l = 0..Ntau, sf_columns(dim) = 4 dim + 2 of them:
  !   B(1:dim,l)           Dcm_k  = C/(S n_pairs(l) Np)            n_pairs(l) = 2 window + 1 - l
  !   B(dim+1:2dim,l)      rhos_k = Dcm_k/(2 lam l dt), 0 at l = 0 (rhos_vpi.out has no line for it)
  !   B(2dim+1,l)          the mean of rhos_k over the axes
  !   B(2dim+2:3dim+1,l)   msd_k  = D/(S n_pairs(l) Np)
  !   B(3dim+2,l)          the sum of msd_k over the axes
  !   B(3dim+3:4dim+2,l)   cross_k = Dcm_k - msd_k
  ! (profiles.normalize_sf has the same expressions)
  integer function sf_columns(dim)
    integer, intent(in) :: dim
    sf_columns = 4*dim+2
  end function sf_columns

  subroutine normalize_sf(dim,Np,Ntau,window,dt,lam,S,C,D,B)
    integer, intent(in)    :: dim,Np,Ntau,window
    real(8), intent(in)    :: dt,lam,C(dim,0:Ntau),D(dim,0:Ntau)
    integer(8), intent(in) :: S
    real(8), intent(out)   :: B(4*dim+2,0:Ntau)
    integer :: l,k
    real(8) :: norm,tau
    do l=0,Ntau
       norm = real(S,8)*real(2*window+1-l,8)*real(Np,8)
       tau  = real(l,8)*dt
       do k=1,dim
          B(k,l) = C(k,l)/norm
          B(dim+k,l) = 0.d0
          if (l>0) B(dim+k,l) = B(k,l)/(2.d0*lam*tau)
          B(2*dim+1+k,l) = D(k,l)/norm
          B(3*dim+2+k,l) = B(k,l)-B(2*dim+1+k,l)
       end do
       B(2*dim+1,l) = sum(B(dim+1:2*dim,l))/real(dim,8)
       B(3*dim+2,l) = sum(B(2*dim+2:3*dim+1,l))
    end do
  end subroutine normalize_sf

  ! rhos_vpi.out: one line per lag l >= 1: tau_l = l dt; Dcm_k and its error over the n blocks, per axis; rhos_k and its
  ! error, per axis; the mean of rhos_k over the axes and its error
  subroutine write_rhos(fname,dim,Ntau,dt,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: dim,Ntau,n
    real(8), intent(in) :: dt,av(4*dim+2,0:Ntau),av2(4*dim+2,0:Ntau)
    integer :: l,j,u
    real(8) :: a(2*dim+1),a2(2*dim+1)
    open (newunit=u,file=fname)
    do l=1,Ntau
       a  = av(1:2*dim+1,l)/real(n)
       a2 = av2(1:2*dim+1,l)/real(n)
       write (u,'(40g20.10e3)') real(l,8)*dt,(a(j),variance(n,a(j),a2(j)),j=1,2*dim+1)
    end do
    close (u)
  end subroutine write_rhos

  ! msdu_vpi.out: one line per lag l >= 0: tau_l; the unfolded msd_k and its error over the n blocks, per axis; their sum
  ! over the axes and its error; cross_k = Dcm_k - msd_k and its error, per axis
  subroutine write_msdu(fname,dim,Ntau,dt,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: dim,Ntau,n
    real(8), intent(in) :: dt,av(4*dim+2,0:Ntau),av2(4*dim+2,0:Ntau)
    integer :: l,j,u
    real(8) :: a(2*dim+1),a2(2*dim+1)
    open (newunit=u,file=fname)
    do l=0,Ntau
       a  = av(2*dim+2:4*dim+2,l)/real(n)
       a2 = av2(2*dim+2:4*dim+2,l)/real(n)
       write (u,'(40g20.10e3)') real(l,8)*dt,(a(j),variance(n,a(j),a2(j)),j=1,2*dim+1)
    end do
    close (u)
  end subroutine write_msdu

  ! ---- clusters (raw sums of pigs_cl_read of one walker and block, S samples = window slices) -> the block values
  !   BS(1,s) n(s) = nsize/S            the clusters of size s per slice
  !   BS(2,s) s n(s)/Np                 the share of the particles in clusters of size s
  !   BS(3,s) nlarge/S                  the probability that the largest cluster has size s
  !   BS(4,s) rg2/S                     the sum of Rg^2 over the clusters of size s, per slice (additive over blocks; <Rg^2>(s)
  !                                     = rg2/nsize, as profiles.normalize_cl has it, is BS(4,s)/BS(1,s))
  !   BB(1) clusters per slice = sum_s n(s);  BB(2) <smax>/Np = sum_s s nlarge/(S Np);  BB(3) the mean cluster size
  !   sum s^2 nsize / sum s nsize;  BB(4) bonds per particle = nbond/(S Np)
  subroutine normalize_cl(Np,S,nsize,nlarge,nbond,rg2,BS,BB)
    integer, intent(in)    :: Np
    integer(8), intent(in) :: S,nsize(Np),nlarge(Np),nbond
    real(8), intent(in)    :: rg2(Np)
    real(8), intent(out)   :: BS(4,Np),BB(4)
    integer :: i
    real(8) :: rs,s1,s2,sl
    rs = real(S,8)
    s1 = 0.d0; s2 = 0.d0; sl = 0.d0
    BB = 0.d0
    do i=1,Np
       BS(1,i) = real(nsize(i),8)/rs
       BS(2,i) = real(i,8)*BS(1,i)/real(Np,8)
       BS(3,i) = real(nlarge(i),8)/rs
       BS(4,i) = rg2(i)/rs
       BB(1) = BB(1)+BS(1,i)
       sl = sl+real(i,8)*real(nlarge(i),8)
       s1 = s1+real(i,8)*real(nsize(i),8)
       s2 = s2+real(i,8)*real(i,8)*real(nsize(i),8)
    end do
    BB(2) = sl/(rs*real(Np,8))
    BB(3) = s2/s1
    BB(4) = real(nbond,8)/(rs*real(Np,8))
  end subroutine normalize_cl

  ! first line of clusblk_vpi*.out
  subroutine clus_header(u,rc,window)
    integer, intent(in) :: u,window
    real(8), intent(in) :: rc
    write (u,'(a,g0,a,i0,a,i0,a)') '# block, clusters per slice (bonds below rc = ',rc,', slices Nb-',window,'..Nb+',window, &
         & '), <largest cluster>/Np, mean cluster size sum s^2 n(s) / sum s n(s), bonds per particle'
  end subroutine clus_header

  ! one line of clusblk_vpi*.out
  subroutine write_clus_block(u,iblock,BB)
    integer, intent(in) :: u,iblock
    real(8), intent(in) :: BB(4)
    write (u,'(20g20.10e3)') real(iblock),BB
  end subroutine write_clus_block

  ! clus_vpi.out: one line per size s that occurred: s; n(s), s n(s)/Np and P_largest(s), each with its error over the n
  ! blocks; <Rg^2>(s) = <rg2/S> / <n(s)>, the two means over the blocks, and the error of its numerator over <n(s)>
  subroutine write_clus(fname,Np,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: Np,n
    real(8), intent(in) :: av(4,Np),av2(4,Np)
    integer :: i,j,u
    real(8) :: a(4),a2(4)
    open (newunit=u,file=fname)
    do i=1,Np
       if (.not. (av(1,i)>0.d0)) cycle
       a  = av(:,i)/real(n)
       a2 = av2(:,i)/real(n)
       write (u,'(i8,20g20.10e3)') i,(a(j),variance(n,a(j),a2(j)),j=1,3),a(4)/a(1),variance(n,a(4),a2(4))/a(1)
    end do
    close (u)
  end subroutine write_clus

  ! ---- percolation (raw sums of pigs_pc_read of one walker and block, S samples = window slices) -> the block values
  !   BB(k) k = 1..3   the share of the slices with a cluster that wraps along axis k (0 beyond dim)
  !   BB(4), BB(5)     the same along any axis and along all dim axes
  !   BB(6)            P_inf = sum_{mask /= 0} mwrap/(Np S), the share of the particles in wrapping clusters
  !   BB(7)            the mean finite cluster size sum s^2 nfin / sum s nfin (0 in a block without a finite cluster)
  !   BS(1,s) nfin/(Np S)   the finite clusters of size s per particle
  !   BS(2,s) rg2u/S        the sum of the unfolded Rg^2 over the finite clusters of size s, per slice (additive over the
  !                         blocks; <Rg^2>(s) = rg2u/nfin, as profiles.normalize_pc has it, is BS(2,s)/(Np BS(1,s)))
  !   BP(1:3,l) first, second, both per origin (/norig): additive over the blocks; C(l) = BP(3)/BP(1)
  subroutine normalize_pc(Np,dim,ntau,S,nwrap,mwrap,swrap,nfin,rg2u,first,second,both,norig,BB,BS,BP)
    integer, intent(in)    :: Np,dim,ntau
    integer(8), intent(in) :: S,nwrap(0:7),mwrap(0:7),swrap(0:7),nfin(Np)
    integer(8), intent(in) :: first(0:ntau),second(0:ntau),both(0:ntau),norig(0:ntau)
    real(8), intent(in)    :: rg2u(Np)
    real(8), intent(out)   :: BB(7),BS(2,Np),BP(3,0:ntau)
    integer :: i,k,m,l
    real(8) :: rs,s1,s2
    rs = real(S,8)
    BB = 0.d0
    do m=1,7
       do k=1,dim
          if (btest(m,k-1)) BB(k) = BB(k)+real(swrap(m),8)/rs
       end do
       BB(4) = BB(4)+real(swrap(m),8)/rs
       BB(6) = BB(6)+real(mwrap(m),8)/(rs*real(Np,8))
    end do
    BB(5) = real(swrap(2**dim-1),8)/rs
    s1 = 0.d0; s2 = 0.d0
    do i=1,Np
       BS(1,i) = real(nfin(i),8)/(rs*real(Np,8))
       BS(2,i) = rg2u(i)/rs
       s1 = s1+real(i,8)*real(nfin(i),8)
       s2 = s2+real(i,8)*real(i,8)*real(nfin(i),8)
    end do
    if (s1>0.d0) BB(7) = s2/s1
    do l=0,ntau
       BP(1,l) = real(first(l),8)/real(norig(l),8)
       BP(2,l) = real(second(l),8)/real(norig(l),8)
       BP(3,l) = real(both(l),8)/real(norig(l),8)
    end do
  end subroutine normalize_pc

  ! first line of perc_vpi*.out
  subroutine perc_header(u,rc,window)
    integer, intent(in) :: u,window
    real(8), intent(in) :: rc
    write (u,'(a,g0,a,i0,a,i0,a)') '# block, wrapping probability along x, y, z (bonds below rc = ',rc,', slices Nb-',window,'..Nb+', &
         & window,'; 0 beyond dim), along any axis, along all axes, P_inf, mean finite cluster size'
  end subroutine perc_header

  ! one line of perc_vpi*.out
  subroutine write_perc_block(u,iblock,BB)
    integer, intent(in) :: u,iblock
    real(8), intent(in) :: BB(7)
    write (u,'(20g20.10e3)') real(iblock),BB
  end subroutine write_perc_block

  ! percsz_vpi.out: one line per finite size s that occurred: s; n_fin(s)/Np with its error over the n blocks; <Rg^2>(s) =
  ! <rg2u/S> / <nfin/S>, the two means over the blocks, and the error of its numerator over <nfin/S>
  subroutine write_percsz(fname,Np,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: Np,n
    real(8), intent(in) :: av(2,Np),av2(2,Np)
    integer :: i,u
    real(8) :: a(2),a2(2)
    open (newunit=u,file=fname)
    do i=1,Np
       if (.not. (av(1,i)>0.d0)) cycle
       a  = av(:,i)/real(n)
       a2 = av2(:,i)/real(n)
       write (u,'(i8,20g20.10e3)') i,a(1),variance(n,a(1),a2(1)),a(2)/(a(1)*real(Np,8)),variance(n,a(2),a2(2))/(a(1)*real(Np,8))
    end do
    close (u)
  end subroutine write_percsz

  ! clpers_vpi.out: one line per lag l: l, tau = l dt, then value and error over the n blocks of the pairs per origin that
  ! are together in slice a, in a+l and in both; the persistence C(l) = <both>/<first> and the Jaccard index
  ! <both>/(<first>+<second>-<both>), ratios of block means (0 where the denominator is 0)
  subroutine write_clpers(fname,ntau,dt,n,av,av2)
    character(len=*), intent(in) :: fname
    integer, intent(in) :: ntau,n
    real(8), intent(in) :: dt,av(3,0:ntau),av2(3,0:ntau)
    integer :: l,j,u
    real(8) :: a(3),a2(3),c,jac
    open (newunit=u,file=fname)
    do l=0,ntau
       a  = av(:,l)/real(n)
       a2 = av2(:,l)/real(n)
       c = 0.d0; jac = 0.d0
       if (a(1)>0.d0) c = a(3)/a(1)
       if (a(1)+a(2)-a(3)>0.d0) jac = a(3)/(a(1)+a(2)-a(3))
       write (u,'(i8,20g20.10e3)') l,real(l,8)*dt,(a(j),variance(n,a(j),a2(j)),j=1,3),c,jac
    end do
    close (u)
  end subroutine write_clpers

  ! grvec_vpi.out: one line per bin in flat-index order (x fastest): r_1..r_dim at the bin centre, g, error over the n blocks
  subroutine write_grvec(fname,p,Ng,nv,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in)    :: Ng,nv,n
    real(8), intent(inout) :: av(nv),av2(nv)
    integer :: j,k,u,rest
    real(8) :: r(3),b
    open (newunit=u,file=fname)
    do j=1,nv
       av(j)  = av(j)/real(n)
       av2(j) = av2(j)/real(n)
       rest = j-1
       do k=1,p%dim
          b    = p%Lbox(k)/real(Ng,8)
          r(k) = -0.5d0*p%Lbox(k)+(real(mod(rest,Ng),8)+0.5d0)*b
          rest = rest/Ng
       end do
       write (u,'(20g20.10e3)') (r(k),k=1,p%dim),av(j),variance(n,av(j),av2(j))
    end do
    close (u)
  end subroutine write_grvec

  ! the reference's "variance": standard error sqrt((<x^2>-<x>^2)/n)
  function variance(n,av,av2) result(v)
    integer, intent(in) :: n
    real(8), intent(in) :: av,av2
    real(8) :: v
    v = sqrt((av2-av*av)/real(n))
  end function variance

  subroutine perm_sampling(ps,isopen,iw,ik,swap_accepted)
    type(perm_state), intent(inout) :: ps
    logical, intent(in) :: isopen
    integer, intent(in) :: iw
    integer, intent(in), optional :: ik
    logical, intent(in), optional :: swap_accepted
    logical :: already
    if (ps%new_cycle) then
       ps%members    = 0
       ps%members(1) = iw
       ps%iperm      = 1
       ps%new_cycle  = .false.
    end if
    if (present(swap_accepted)) then
       if (swap_accepted) then
          already = any(ps%members==ik)
          if (.not. ps%end_cycle) then
             if (.not. already) then
                ps%iperm = ps%iperm+1
                ps%members(ps%iperm) = ik
             end if
          end if
       end if
    end if
    if (ps%end_cycle) then
       ps%histogram(ps%iperm) = ps%histogram(ps%iperm)+1
       if (isopen) then
          ps%members    = 0
          ps%members(1) = iw
          ps%iperm      = 1
       end if
       ps%end_cycle = .false.
    end if
  end subroutine perm_sampling

  ! ---- output files (formats of the reference)
  subroutine write_radial(fname,p,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in) :: n
    real(8), intent(inout) :: av(p%Nbin),av2(p%Nbin)
    real(8) :: r
    integer :: j,u
    open (newunit=u,file=fname)
    do j=1,p%Nbin
       r      = (real(j)-0.5d0)*p%rbin
       av(j)  = av(j)/real(n)
       av2(j) = av2(j)/real(n)
       write (u,'(20g20.10e3)') r,av(j),variance(n,av(j),av2(j))
    end do
    close (u)
  end subroutine write_radial

  subroutine write_sk(fname,p,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in) :: n
    real(8), intent(inout) :: av(p%dim,p%Nk),av2(p%dim,p%Nk)
    integer :: j,k,u
    open (newunit=u,file=fname)
    do j=1,p%Nk
       av(:,j)  = av(:,j)/real(n)
       av2(:,j) = av2(:,j)/real(n)
       write (u,'(20g20.10e3)') (j*p%qbin(k),av(k,j),variance(n,av(k,j),av2(k,j)),k=1,p%dim)
    end do
    close (u)
  end subroutine write_sk

  subroutine write_nr(fname,p,n,av,av2)
    character(len=*), intent(in) :: fname
    type(est_params), intent(in) :: p
    integer, intent(in) :: n
    real(8), intent(inout) :: av(0:p%Npw,p%Nbin),av2(0:p%Npw,p%Nbin)
    real(8) :: r
    integer :: j,m,u
    open (newunit=u,file=fname)
    do j=1,p%Nbin
       r = (real(j)-0.5d0)*p%rbin
       av(:,j)  = av(:,j)/real(n)
       av2(:,j) = av2(:,j)/real(n)
       write (u,'(20g20.10e3)') r,(av(m,j),variance(n,av(m,j),av2(m,j)),m=0,p%Npw)
    end do
    close (u)
  end subroutine write_nr

end module pigs_estimators
