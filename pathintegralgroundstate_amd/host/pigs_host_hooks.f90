!-----------------------------------------------------------------------
! pigs_host_hooks -- C-callable handles on the host sampler (state in / state out), so that
! its logic can be driven and inspected from outside Fortran: tests compare every mover,
! on identical random-number state, with the reference's own routine.
!-----------------------------------------------------------------------
module pigs_host_hooks

  use iso_c_binding
  use pigs_capi
  use pigs_rng
  use pigs_sampler
  use pigs_estimators, only: est_params, normalize_vh, write_vh, normalize_g3, write_g3, write_g3ang, &
       & normalize_atm, atm_window_mean, v3_header, write_v3_block, write_v3tau, &
       & normalize_lat, lind_header, write_lind_block, write_lindtau, write_usite, &
       & normalize_sf, sf_columns, write_rhos, write_msdu, &
       & normalize_cl, clus_header, write_clus_block, write_clus, &
       & normalize_pc, perc_header, write_perc_block, write_percsz, write_clpers, &
       & normalize_nk, normalize_nrvec, n0_header, write_n0_block, write_nkvec, write_sqshell, write_grvec, &
       & sqv_shells, sqv_shell_means

  implicit none
  private

  integer, parameter :: MAXS = 16
  type(sampler_t), target, save :: pool(MAXS)
  logical, save :: used(MAXS) = .false.

contains

  function hs_create(dim,Np,Nb,W,trap,dt,density,CWorm,Lbox,ctx) bind(C,name='hs_create') result(h)
    integer(c_int), value :: dim,Np,Nb,W,trap
    real(c_double), value :: dt,density,CWorm
    real(c_double), intent(in) :: Lbox(dim)
    type(c_ptr), value :: ctx
    integer(c_int) :: h
    integer :: i
    h = -1
    do i=1,MAXS
       if (.not. used(i)) then
          used(i) = .true.
          call sampler_init(pool(i),dim,Np,Nb,W,trap/=0,dt,density,CWorm,Lbox,ctx)
          h = i
          return
       end if
    end do
  end function hs_create

  subroutine hs_destroy(h) bind(C,name='hs_destroy')
    integer(c_int), value :: h
    if (h<1 .or. h>MAXS) return
    if (used(h)) call sampler_free(pool(h))
    used(h) = .false.
  end subroutine hs_destroy

  subroutine hs_set_path(h,w,P) bind(C,name='hs_set_path')
    integer(c_int), value :: h,w
    real(c_double), intent(in) :: P(*)
    integer :: n
    n = size(pool(h)%Path(:,:,:,1))
    pool(h)%Path(:,:,:,w+1) = reshape(P(1:n),shape(pool(h)%Path(:,:,:,1)))
  end subroutine hs_set_path

  subroutine hs_get_path(h,w,P) bind(C,name='hs_get_path')
    integer(c_int), value :: h,w
    real(c_double) :: P(*)
    integer :: n
    n = size(pool(h)%Path(:,:,:,1))
    P(1:n) = reshape(pool(h)%Path(:,:,:,w+1),[n])
  end subroutine hs_get_path

  subroutine hs_upload(h) bind(C,name='hs_upload')
    integer(c_int), value :: h
    call sampler_upload(pool(h))
  end subroutine hs_upload

  subroutine hs_flush(h) bind(C,name='hs_flush')
    integer(c_int), value :: h
    call sampler_flush(pool(h))
  end subroutine hs_flush

  subroutine hs_seed(h,w,seed) bind(C,name='hs_seed')
    integer(c_int), value :: h,w,seed
    call mt_seed(pool(h)%rng(w+1),seed)
  end subroutine hs_seed

  subroutine hs_set_rng(h,w,pos,words) bind(C,name='hs_set_rng')
    integer(c_int), value :: h,w,pos
    integer(c_int32_t), intent(in) :: words(0:623)
    pool(h)%rng(w+1)%pos = pos
    pool(h)%rng(w+1)%w   = words
  end subroutine hs_set_rng

  subroutine hs_get_rng(h,w,pos,words) bind(C,name='hs_get_rng')
    integer(c_int), value :: h,w
    integer(c_int) :: pos
    integer(c_int32_t) :: words(0:623)
    pos   = pool(h)%rng(w+1)%pos
    words = pool(h)%rng(w+1)%w
  end subroutine hs_get_rng

  subroutine hs_set_worm(h,w,isopen,iworm,xend) bind(C,name='hs_set_worm')
    integer(c_int), value :: h,w,isopen,iworm
    real(c_double), intent(in) :: xend(*)
    integer :: d
    d = pool(h)%dim
    pool(h)%isopen(w+1) = isopen/=0
    pool(h)%iworm(w+1)  = iworm
    pool(h)%xend(:,:,w+1) = reshape(xend(1:2*d),[d,2])
  end subroutine hs_set_worm

  subroutine hs_get_worm(h,w,isopen,iworm,xend) bind(C,name='hs_get_worm')
    integer(c_int), value :: h,w
    integer(c_int) :: isopen,iworm
    real(c_double) :: xend(*)
    integer :: d
    d = pool(h)%dim
    isopen = merge(1,0,pool(h)%isopen(w+1))
    iworm  = pool(h)%iworm(w+1)
    xend(1:2*d) = reshape(pool(h)%xend(:,:,w+1),[2*d])
  end subroutine hs_get_worm

  ! code: 1 TranslateChain(rpar=delta) 2 Bisection(i1=level) 3 MoveHeadBisection 4 MoveTailBisection
  !       5 Staging(i1=Lstag) 6 MoveHead(i1=Lmax) 7 MoveTail
  !       8 TranslateHalfChain(i2=half,rpar=delta) 9 StagingHalfChain(i1=Lstag,i2=half)
  !       10 MoveHeadHalfChain(i1=Lmax,i2=half) 11 MoveTailHalfChain
  !       12 OpenChain(i1=Lmax) 13 CloseChain(i1=Lmax) 14 Swap(i1=Lmax; partner/swapped out)
  subroutine hs_move(h,code,i1,i2,rpar,ip_of,active,accepted,partner,swapped) bind(C,name='hs_move')
    integer(c_int), value :: h,code,i1,i2
    real(c_double), value :: rpar
    integer(c_int), intent(in) :: ip_of(*),active(*)
    integer(c_int) :: accepted(*),partner(*),swapped(*)
    integer :: W
    integer, allocatable :: ipo(:),acc(:),par(:)
    logical, allocatable :: act(:),swp(:)
    W = pool(h)%W
    allocate(ipo(W),acc(W),par(W),act(W),swp(W))
    ipo = ip_of(1:W); act = active(1:W)/=0; acc = accepted(1:W); par = 0; swp = .false.
    select case (code)
    case (1);  call mv_translate(pool(h),rpar,ipo,act,acc)
    case (2);  call mv_bisection(pool(h),i1,ipo,act,acc)
    case (3);  call mv_end_bisection(pool(h),HEAD,i1,ipo,act,acc)
    case (4);  call mv_end_bisection(pool(h),TAIL,i1,ipo,act,acc)
    case (5);  call mv_staging(pool(h),i1,ipo,act,acc)
    case (6);  call mv_end_staging(pool(h),HEAD,i1,ipo,act,acc)
    case (7);  call mv_end_staging(pool(h),TAIL,i1,ipo,act,acc)
    case (8);  call mv_translate_half(pool(h),i2,rpar,act,acc)
    case (9);  call mv_staging_half(pool(h),i2,i1,act,acc)
    case (10); call mv_end_staging_half(pool(h),HEAD,i2,i1,act,acc)
    case (11); call mv_end_staging_half(pool(h),TAIL,i2,i1,act,acc)
    case (12); call mv_open(pool(h),i1,ipo,act,acc)
    case (13); call mv_close(pool(h),i1,act,acc)
    case (14); call mv_swap(pool(h),i1,act,acc,par,swp)
    end select
    accepted(1:W) = acc
    partner(1:W)  = par
    swapped(1:W)  = merge(1,0,swp)
  end subroutine hs_move

  subroutine hs_uniform_stream(seed,n,u) bind(C,name='hs_uniform_stream')
    integer(c_int), value :: seed,n
    real(c_double) :: u(n)
    type(mt_state) :: st
    integer :: i
    call mt_seed(st,seed)
    do i=1,n
       u(i) = mt_real(st)
    end do
  end subroutine hs_uniform_stream

  subroutine hs_gauss_stream(seed,n,g) bind(C,name='hs_gauss_stream')
    integer(c_int), value :: seed,n
    real(c_double) :: g(n)
    type(mt_state) :: st
    integer :: i
    call mt_seed(st,seed)
    do i=1,n
       call mt_gauss(st,g(i))
    end do
  end subroutine hs_gauss_stream

  ! The van Hove normalisation and writers of the front end on given counts: nb blocks of one walker, cself
  ! (Ns,0:Ntau,nb), cdist (Nr,0:Ntau,nb) and S samples per block -> gs, gd of the LAST block, and the two files with the
  ! mean and error over the blocks (names: C strings)
  subroutine hs_vh_files(dim,Np,density,window,Ntau,Nr,rbin,Ns,sbin,dt,nb,S,cself,cdist,gs,gd,fd,fs) bind(C,name='hs_vh_files')
    integer(c_int), value :: dim,Np,window,Ntau,Nr,Ns,nb
    real(c_double), value :: density,rbin,sbin,dt
    integer(c_int64_t), intent(in) :: S(nb),cself(Ns,0:Ntau,nb),cdist(Nr,0:Ntau,nb)
    real(c_double), intent(out)    :: gs(Ns,0:Ntau),gd(Nr,0:Ntau)
    character(kind=c_char), intent(in) :: fd(*),fs(*)
    type(est_params) :: p,ps
    real(8), allocatable :: ad(:,:),ad2(:,:),as(:,:),as2(:,:)
    integer :: b
    p%dim = dim; p%Np = Np; p%Nbin = Nr; p%rbin = rbin; p%pi = acos(-1.d0)
    ps = p
    ps%Nbin = Ns; ps%rbin = sbin
    allocate (ad(Nr,0:Ntau),ad2(Nr,0:Ntau),as(Ns,0:Ntau),as2(Ns,0:Ntau))
    ad = 0.d0; ad2 = 0.d0; as = 0.d0; as2 = 0.d0
    do b=1,nb
       call normalize_vh(p,ps,density,window,int(S(b),8),Ntau,cself(:,:,b),cdist(:,:,b),gs,gd)
       ad = ad+gd; ad2 = ad2+gd*gd
       as = as+gs; as2 = as2+gs*gs
    end do
    call write_vh(cstring(fd),p,dt,Ntau,nb,ad,ad2)
    call write_vh(cstring(fs),ps,dt,Ntau,nb,as,as2)
  end subroutine hs_vh_files

  ! The triplet normalisation and writers of the front end on given counts: nb blocks of one walker, ctrip
  ! (Na,Nr(Nr+1)/2,nb), cpair (Nr,nb) and S samples per block -> g2, g3, pang of the LAST block, and the two files with the
  ! mean and error over the blocks (names: C strings)
  subroutine hs_g3_files(dim,Np,density,window,Nr,rbin,Na,nb,S,ctrip,cpair,g2,g3,pang,f3,fa) bind(C,name='hs_g3_files')
    integer(c_int), value :: dim,Np,window,Nr,Na,nb
    real(c_double), value :: density,rbin
    integer(c_int64_t), intent(in) :: S(nb),ctrip(Na,Nr*(Nr+1)/2,nb),cpair(Nr,nb)
    real(c_double), intent(out)    :: g2(Nr),g3(Na,Nr*(Nr+1)/2),pang(Na)
    character(kind=c_char), intent(in) :: f3(*),fa(*)
    type(est_params) :: p
    real(8), allocatable :: a3(:,:),a32(:,:),aa(:),aa2(:)
    integer :: b
    p%dim = dim; p%Np = Np; p%Nbin = Nr; p%rbin = rbin; p%pi = acos(-1.d0)
    allocate (a3(Na,Nr*(Nr+1)/2),a32(Na,Nr*(Nr+1)/2),aa(Na),aa2(Na))
    a3 = 0.d0; a32 = 0.d0; aa = 0.d0; aa2 = 0.d0
    do b=1,nb
       call normalize_g3(p,density,window,int(S(b),8),Na,ctrip(:,:,b),cpair(:,b),g2,g3,pang)
       a3 = a3+g3; a32 = a32+g3*g3
       aa = aa+pang; aa2 = aa2+pang*pang
    end do
    call write_g3(cstring(f3),p,Na,nb,a3,a32)
    call write_g3ang(cstring(fa),Na,nb,aa,aa2)
  end subroutine hs_g3_files

  ! The three-body normalisation and writers of the front end on given sums: nblk blocks of one walker, T and ntrip
  ! (2 window + 1,nblk) and S samples per block, the coupling nu -> v3, cnt of the LAST block and its window mean, and the two
  ! files: fb one line per block (v3_vpi.out), ft mean and error over the blocks per slice (v3tau_vpi.out) (names: C strings)
  subroutine hs_atm_files(dim,Np,density,Nb,window,dt,nu,nblk,S,T,ntrip,v3,cnt,v3mean,fb,ft) bind(C,name='hs_atm_files')
    integer(c_int), value :: dim,Np,Nb,window,nblk
    real(c_double), value :: density,dt,nu
    integer(c_int64_t), intent(in) :: S(nblk),ntrip(2*window+1,nblk)
    real(c_double), intent(in)     :: T(2*window+1,nblk)
    real(c_double), intent(out)    :: v3(2*window+1),cnt(2*window+1),v3mean
    character(kind=c_char), intent(in) :: fb(*),ft(*)
    real(8), allocatable :: B(:,:),a(:,:),a2(:,:)
    integer :: ib,u
    allocate (B(2,2*window+1),a(2,2*window+1),a2(2,2*window+1))
    a = 0.d0; a2 = 0.d0
    open (newunit=u,file=cstring(fb))
    call v3_header(u,window)
    do ib=1,nblk
       call normalize_atm(Np,window,nu,int(S(ib),8),T(:,ib),int(ntrip(:,ib),8),B)
       a = a+B; a2 = a2+B*B
       v3mean = atm_window_mean(window,B)
       call write_v3_block(u,ib,dim,density,v3mean)
    end do
    close (u)
    v3 = B(1,:); cnt = B(2,:)
    call write_v3tau(cstring(ft),Nb,window,dt,nblk,a,a2)
  end subroutine hs_atm_files

  ! The momentum-distribution normalisation and writers of the front end on given sums: nblk blocks of one walker, cosine
  ! sums C (Nq,nblk) on the vectors nvq (dim,Nq), counts H (nbin**dim,nblk), nopen and zconf per block -> nk (0:Nq) and rho1 of
  ! the LAST block, and the four files (names: C strings): fv per vector, fs per shell, f0 per block, fr per bin
  subroutine hs_nk_files(dim,Np,Lbox,density,cworm,Nobdm,Nq,nvq,nbin,nblk,zconf,C,nopen,H,nk,rho1,fv,fs,f0,fr) &
       & bind(C,name='hs_nk_files')
    integer(c_int), value :: dim,Np,Nobdm,Nq,nbin,nblk
    real(c_double), value :: density,cworm
    real(c_double), intent(in)     :: Lbox(dim),zconf(nblk),C(Nq,nblk)
    integer(c_int32_t), intent(in) :: nvq(dim,Nq)
    integer(c_int64_t), intent(in) :: nopen(nblk),H(nbin**dim,nblk)
    real(c_double), intent(out)    :: nk(0:Nq),rho1(nbin**dim)
    character(kind=c_char), intent(in) :: fv(*),fs(*),f0(*),fr(*)
    type(est_params) :: p
    real(8), allocatable :: a(:),a2(:),ar(:),ar2(:),sh(:),as(:),as2(:),q(:)
    integer, allocatable :: shell(:),mult(:)
    integer :: ib,u,nsh,nv
    p%dim = dim; p%Np = Np; p%pi = acos(-1.d0); p%CWorm = cworm
    p%Lbox = 1.d0; p%Lbox(1:dim) = Lbox; p%LboxHalf = 0.5d0*p%Lbox; p%qbin = 2.d0*p%pi/p%Lbox
    nv = nbin**dim
    allocate (shell(Nq))
    call sqv_shells(p,Nq,nvq,shell,nsh,q,mult)
    allocate (a(0:Nq),a2(0:Nq),ar(nv),ar2(nv),sh(nsh),as(nsh),as2(nsh))
    a = 0.d0; a2 = 0.d0; ar = 0.d0; ar2 = 0.d0; as = 0.d0; as2 = 0.d0
    open (newunit=u,file=cstring(f0))
    call n0_header(u)
    do ib=1,nblk
       call normalize_nk(cworm,zconf(ib),Nobdm,Nq,C(:,ib),int(nopen(ib),8),nk)
       call sqv_shell_means(Nq,shell,nsh,mult,nk(1:),sh)
       call normalize_nrvec(p,cworm,zconf(ib),Nobdm,density,nbin,nv,int(H(:,ib),8),rho1)
       a = a+nk; a2 = a2+nk*nk
       as = as+sh; as2 = as2+sh*sh
       ar = ar+rho1; ar2 = ar2+rho1*rho1
       call write_n0_block(u,ib,Np,nk(0))
    end do
    close (u)
    call write_nkvec(cstring(fv),p,Nq,nvq,nblk,a,a2)
    call write_sqshell(cstring(fs),nsh,q,mult,nblk,as,as2)
    call write_grvec(cstring(fr),p,nbin,nv,nblk,ar,ar2)
  end subroutine hs_nk_files

  ! The lattice normalisation and writers of the front end on given sums: nblk blocks of one walker, the arrays of
  ! pigs_lat_read per block and S samples per block -> the three files: fl one line per block (lind_vpi.out), ft the means
  ! over the blocks per window slice (lindtau_vpi.out), fu per bin (usite_vpi.out) (names: C strings)
  subroutine hs_lat_files(dim,Np,nsite,window,nbin,dt,ann,rmax,nblk,S,mom,nass,occ,hr,hx,hop1,hopw,fl,ft,fu) &
       & bind(C,name='hs_lat_files')
    integer(c_int), value :: dim,Np,nsite,window,nbin,nblk
    real(c_double), value :: dt,ann,rmax
    integer(c_int64_t), intent(in) :: S(nblk),nass(2*window+1,nblk),occ(4,2*window+1,nblk),hr(nbin,nblk),hx(2*nbin,dim,nblk)
    integer(c_int64_t), intent(in) :: hop1(nblk),hopw(nblk)
    real(c_double), intent(in)     :: mom(2+dim,2*window+1,nblk)
    character(kind=c_char), intent(in) :: fl(*),ft(*),fu(*)
    real(8), allocatable :: BT(:,:),BU(:),aT(:,:),aU(:)
    real(8) :: BL(7)
    integer :: ib,u
    allocate (BT(2+dim,2*window+1),aT(2+dim,2*window+1),BU(nbin*(1+2*dim)),aU(nbin*(1+2*dim)))
    aT = 0.d0; aU = 0.d0
    open (newunit=u,file=cstring(fl))
    call lind_header(u,window)
    do ib=1,nblk
       call normalize_lat(dim,Np,nsite,window,nbin,ann,rmax,acos(-1.d0),int(S(ib),8),mom(:,:,ib),int(nass(:,ib),8), &
            & int(occ(:,:,ib),8),int(hr(:,ib),8),int(hx(:,:,ib),8),int(hop1(ib),8),int(hopw(ib),8),BL,BT,BU)
       aT = aT+BT; aU = aU+BU
       call write_lind_block(u,ib,BL)
    end do
    close (u)
    call write_lindtau(cstring(ft),dim,window,dt,nblk,aT)
    call write_usite(cstring(fu),dim,nbin,rmax,nblk,aU)
  end subroutine hs_lat_files

  ! The centre-of-mass diffusion normalisation and writers of the front end on given sums: nblk blocks of one walker, C and
  ! D of pigs_sf_read per block and S samples per block -> fr (rhos_vpi.out) and fm (msdu_vpi.out), the means and errors
  ! over the blocks through a block_series, as the front end takes them (names: C strings)
  subroutine hs_sf_files(dim,Np,Ntau,window,dt,lam,nblk,S,C,D,fr,fm) bind(C,name='hs_sf_files')
    use pigs_block_stats, only: block_series,series_create,series_add
    integer(c_int), value :: dim,Np,Ntau,window,nblk
    real(c_double), value :: dt,lam
    integer(c_int64_t), intent(in) :: S(nblk)
    real(c_double), intent(in)     :: C(dim,Ntau+1,nblk),D(dim,Ntau+1,nblk)     ! (second index: lag l + 1)
    character(kind=c_char), intent(in) :: fr(*),fm(*)
    real(8), allocatable :: B(:,:)
    real(8) :: none(1)
    type(block_series) :: sr
    integer :: ib,nq
    nq = sf_columns(dim)
    allocate (B(nq,Ntau+1))
    call series_create(sr,nq*(Ntau+1),1)
    do ib=1,nblk
       call normalize_sf(dim,Np,Ntau,window,dt,lam,int(S(ib),8),C(:,:,ib),D(:,:,ib),B)
       call series_add(sr,1,reshape(B,[size(B)]),none)
    end do
    call write_rhos(cstring(fr),dim,Ntau,dt,nblk,sr%sum(:,1),sr%sq(:,1))
    call write_msdu(cstring(fm),dim,Ntau,dt,nblk,sr%sum(:,1),sr%sq(:,1))
  end subroutine hs_sf_files

  ! The cluster normalisation and writers of the front end on given sums: nblk blocks of one walker, the arrays of
  ! pigs_cl_read per block and S samples per block -> fc (clus_vpi.out) and fb (clusblk_vpi.out), the means and errors over
  ! the blocks through a block_series, as the front end takes them (names: C strings)
  subroutine hs_cl_files(Np,window,rc,nblk,S,nsize,nlarge,nbond,rg2,fc,fb) bind(C,name='hs_cl_files')
    use pigs_block_stats, only: block_series,series_create,series_add
    integer(c_int), value :: Np,window,nblk
    real(c_double), value :: rc
    integer(c_int64_t), intent(in) :: S(nblk),nsize(Np,nblk),nlarge(Np,nblk),nbond(nblk)
    real(c_double), intent(in)     :: rg2(Np,nblk)
    character(kind=c_char), intent(in) :: fc(*),fb(*)
    real(8), allocatable :: BS(:,:)
    real(8) :: BB(4),none(1)
    type(block_series) :: sr
    integer :: ib,u
    allocate (BS(4,Np))
    call series_create(sr,4*Np,1)
    open (newunit=u,file=cstring(fb))
    call clus_header(u,rc,window)
    do ib=1,nblk
       call normalize_cl(Np,int(S(ib),8),int(nsize(:,ib),8),int(nlarge(:,ib),8),int(nbond(ib),8),rg2(:,ib),BS,BB)
       call series_add(sr,1,reshape(BS,[size(BS)]),none)
       call write_clus_block(u,ib,BB)
    end do
    close (u)
    call write_clus(cstring(fc),Np,nblk,sr%sum(:,1),sr%sq(:,1))
  end subroutine hs_cl_files

  ! The percolation normalisation and writers of the front end on given sums: nblk blocks of one walker, the arrays of
  ! pigs_pc_read per block and S samples per block -> fb (perc_vpi.out), fs (percsz_vpi.out) and fp (clpers_vpi.out), the
  ! means and errors over the blocks through block_series, as the front end takes them (names: C strings)
  subroutine hs_pc_files(Np,dim,window,ntau,rc,dt,nblk,S,nwrap,mwrap,swrap,nfin,rg2u,first,second,both,norig,fb,fs,fp) &
       & bind(C,name='hs_pc_files')
    use pigs_block_stats, only: block_series,series_create,series_add
    integer(c_int), value :: Np,dim,window,ntau,nblk
    real(c_double), value :: rc,dt
    integer(c_int64_t), intent(in) :: S(nblk),nwrap(8,nblk),mwrap(8,nblk),swrap(8,nblk),nfin(Np,nblk)
    integer(c_int64_t), intent(in) :: first(ntau+1,nblk),second(ntau+1,nblk),both(ntau+1,nblk),norig(ntau+1,nblk)
    real(c_double), intent(in)     :: rg2u(Np,nblk)
    character(kind=c_char), intent(in) :: fb(*),fs(*),fp(*)
    real(8), allocatable :: BS(:,:),BP(:,:)
    real(8) :: BB(7),none(1)
    type(block_series) :: ss,sp
    integer :: ib,u
    allocate (BS(2,Np),BP(3,ntau+1))                                 ! (second index: lag l + 1)
    call series_create(ss,2*Np,1)
    call series_create(sp,3*(ntau+1),1)
    open (newunit=u,file=cstring(fb))
    call perc_header(u,rc,window)
    do ib=1,nblk
       call normalize_pc(Np,dim,ntau,int(S(ib),8),int(nwrap(:,ib),8),int(mwrap(:,ib),8),int(swrap(:,ib),8),int(nfin(:,ib),8), &
            & rg2u(:,ib),int(first(:,ib),8),int(second(:,ib),8),int(both(:,ib),8),int(norig(:,ib),8),BB,BS,BP)
       call series_add(ss,1,reshape(BS,[size(BS)]),none)
       call series_add(sp,1,reshape(BP,[size(BP)]),none)
       call write_perc_block(u,ib,BB)
    end do
    close (u)
    call write_percsz(cstring(fs),Np,nblk,ss%sum(:,1),ss%sq(:,1))
    call write_clpers(cstring(fp),ntau,dt,nblk,sp%sum(:,1),sp%sq(:,1))
  end subroutine hs_pc_files

  ! a C string as a Fortran one
  function cstring(c) result(f)
    character(kind=c_char), intent(in) :: c(*)
    character(len=:), allocatable :: f
    integer :: n,i
    n = 0
    do while (c(n+1)/=c_null_char)
       n = n+1
    end do
    allocate (character(len=n) :: f)
    do i=1,n
       f(i:i) = c(i)
    end do
  end function cstring

end module pigs_host_hooks
